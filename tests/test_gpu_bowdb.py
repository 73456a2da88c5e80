"""The BoW keyframe database on the device (csrc/bow_db.hip, openvslam_amd.bow.bow_database, cpp/openvslam/data/bow_database.h) against the
sequential reference tests/bowdb_ref.py: scores as uint64 bit patterns, shared-word counts, survivors and candidate lists for equality."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import bowdb_ref
from test_bowdb_ref import N_PLACES, PER_PLACE, loop_query, places_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
MAX_WORDS = 4096
BIG = 1 << 20


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def same(got, want):
    """[(keyframe id, num_common, score)] equal, the scores bit for bit."""
    return [(k, n, bits(s)) for k, n, s in got] == [(k, n, bits(s)) for k, n, s in want]


def normalised(rng, words):
    words = sorted(words)
    weights = [rng.uniform(0.5, 9.0) for _ in words]
    norm = 0.0
    for w in weights:
        norm += abs(w)
    return {w: v / norm for w, v in zip(words, weights)}


@pytest.fixture(scope="module")
def bow():
    from openvslam_amd import bow
    return bow


@pytest.fixture(scope="module")
def places(bow):
    """The "places" scene in a device database and in the reference, built once."""
    vecs, cov = places_scene()
    db, ref = bow.bow_database(64, max_words=512), bowdb_ref.bow_database()
    for kid in sorted(vecs):
        db.add_keyframe(kid, vecs[kid])
        ref.add_keyframe(kid, vecs[kid])
    return vecs, cov, db, ref


# ---- score_all: vector lengths, query lengths, hit positions
@pytest.fixture(scope="module")
def big_db(bow):
    return bow.bow_database(32, max_words=MAX_WORDS)


@pytest.mark.parametrize("nq", [1, 64, 65, MAX_WORDS])
def test_score_all_lengths_and_hit_positions(big_db, nq):
    rng = random.Random(1000 + nq)
    universe = rng.sample(range(1, BIG), 3 * MAX_WORDS)
    q_pool, filler = universe[:MAX_WORDS + 64], sorted(universe[MAX_WORDS + 64:])   # fillers are never query words
    if nq == 1:
        q_words = [q_pool[0]]
    else:
        q_words = [0, BIG] + q_pool[:nq - 2]                                         # word ids 0 and 2^20 are query words
    q = normalised(rng, q_words)
    lo, hi, mid = min(q), max(q), sorted(q)[len(q) // 2]
    below = lambda w, n: [f for f in filler if f < w][-n:] if n else []
    above = lambda w, n: [f for f in filler if f > w][:n] + list(range(BIG + 1, BIG + 1 + n))
    kfs = {}
    for i, length in enumerate((0, 1, 63, 64, 65, 129, MAX_WORDS)):                  # vector lengths; common words by chance
        kfs[100 + i] = normalised(rng, rng.sample(q_pool + filler + [0, BIG], length))
    kfs[200] = dict(q)                                                               # a hit at every entry
    kfs[201] = normalised(rng, [lo] + above(lo, 129)[:129])                          # a hit at the first entry only
    kfs[202] = normalised(rng, below(hi, 129) + [hi])                                # a hit at the last entry only
    kfs[203] = normalised(rng, rng.sample(filler, 150))                              # no hit
    kfs[204] = normalised(rng, below(mid, 150) + [mid] + above(mid, 49)[:49])        # its one hit in round 2, the others' hits in round 0
    kfs[205] = normalised(rng, [0, BIG] + rng.sample(filler, 70))
    assert len(kfs[201]) == 130 and len(kfs[204]) == 200 and len(kfs[202]) >= 2 and len(kfs[100 + 6]) == MAX_WORDS
    assert sorted(kfs[204]).index(mid) >= 128 and sorted(kfs[201])[0] == lo and sorted(kfs[202])[-1] == hi
    ref = bowdb_ref.bow_database()
    big_db.clear()
    for kid in sorted(kfs):
        big_db.add_keyframe(kid, kfs[kid])
        ref.add_keyframe(kid, kfs[kid])
    assert len(big_db) == len(kfs)
    want = ref.score_all(q)
    got = big_db.score_all(q)
    by_id = {k: (n, s) for k, n, s in want}
    assert by_id[200][0] == nq and by_id[201][0] == 1 and by_id[202][0] == 1 and by_id[203] == (0, 0.0) and by_id[204][0] == 1
    assert by_id[100] == (0, 0.0)
    assert [(k, n) for k, n, _ in got] == [(k, n) for k, n, _ in want]
    assert same(got, want)
    # the same through the gated query, and with the full-length keyframe as the query
    assert big_db.query(q) == ref.query(q) and same(big_db.query(q)[0], ref.query(q)[0])
    q2 = kfs[106]
    assert same(big_db.score_all(q2), ref.score_all(q2))
    assert same(big_db.score_all({}), ref.score_all({}))


def test_slot_bookkeeping_erase_and_reuse(bow):
    rng = random.Random(7)
    n = 2049
    db, ref = bow.bow_database(n, max_words=8), bowdb_ref.bow_database()
    vecs = {kid: normalised(rng, rng.sample(range(64), 8)) for kid in range(n)}
    for kid in range(n):
        db.add_keyframe(kid, vecs[kid])
        ref.add_keyframe(kid, vecs[kid])
    q = normalised(rng, rng.sample(range(64), 8))
    assert same(db.score_all(q), ref.score_all(q))
    erased = list(range(0, n, 3))
    for kid in erased:
        db.erase_keyframe(kid)
        ref.erase_keyframe(kid)
    assert len(db) == len(ref) == n - len(erased)
    assert same(db.score_all(q), ref.score_all(q))
    for i, kid in enumerate(erased[::2]):          # half of them come back under new ids, into the freed slots
        vec = normalised(rng, rng.sample(range(64), 1 + i % 8))
        db.add_keyframe(5000 + kid, vec)
        ref.add_keyframe(5000 + kid, vec)
    got = db.score_all(q)
    assert same(got, ref.score_all(q)) and len(got) == len(db) == len(ref)
    assert not set(erased) & {k for k, _, _ in got}
    surv, max_common = db.query(q)
    want, want_max = ref.query(q)
    assert max_common == want_max and same(surv, want) and not set(erased) & {k for k, _, _ in surv}
    db.clear()
    assert len(db) == 0 and db.score_all(q) == [] and db.query(q) == ([], 0)
    db.add_keyframe(1, vecs[1])
    assert same(db.score_all(q), [(1,) + bowdb_ref.score(q, vecs[1])[::-1]])


def test_query_reject_sets(places):
    vecs, cov, db, ref = places
    for qry in (0, 13, 47):
        q = vecs[qry]
        full = ref.score_all(q)
        runner_up = max((n, k) for k, n, _ in full if k != qry)[1]
        for reject in ([], [qry], [qry, runner_up], [qry] + cov(qry), [qry, 9999], sorted(vecs)):
            got, got_max = db.query(q, reject)
            want, want_max = ref.query(q, reject)
            assert got_max == want_max and same(got, want), (qry, reject)
            assert [k for k, _, _ in got] == sorted(k for k, _, _ in got) and not set(reject) & {k for k, _, _ in got}
        # rejecting the holder of max_common lowers the gate: the maximum is taken over what remains
        assert ref.query(q)[1] == len(q) and ref.query(q, [qry])[1] < len(q)
        assert len(ref.query(q, [qry])[0]) > len(ref.query(q)[0])


def test_places_candidates(places):
    vecs, cov, db, ref = places
    for place in range(N_PLACES):
        qry, vec, connected, min_score = loop_query(vecs, cov, place)
        want = ref.acquire_loop_candidates(qry, vec, connected, cov, min_score)
        assert db.acquire_loop_candidates(qry, vec, connected, cov, min_score) == want and want
        want = ref.acquire_relocalization_candidates(vec, cov)
        assert db.acquire_relocalization_candidates(vec, cov) == want and want


def test_determinism_around_an_unrelated_add_and_erase(places):
    vecs, cov, db, ref = places
    q = vecs[21]
    first = db.score_all(q)
    first_q = db.query(q, [21])
    db.add_keyframe(900, vecs[3])
    db.erase_keyframe(900)
    assert same(db.score_all(q), first) and db.query(q, [21])[1] == first_q[1] and same(db.query(q, [21])[0], first_q[0])
    assert same(first, ref.score_all(q))


# ---- end to end: descriptors -> vocabulary.transform -> database -> acquire_*
def _place_descriptors(voc, n_places=3, per_place=4, n_desc=150, seed=5):
    from openvslam_amd.synth import flip_bits
    rng = np.random.Generator(np.random.PCG64(seed))
    leaves = np.nonzero(voc["word_id"] >= 0)[0]
    out = {}
    for place in range(n_places):
        base = voc["desc"][rng.choice(leaves, n_desc, replace=False)]     # words of this place: leaf descriptors
        for j in range(per_place):
            out[place * per_place + j] = np.stack([flip_bits(rng, d, 6) for d in base[rng.permutation(n_desc)[:120]]])
    return out


@pytest.fixture(scope="module")
def vocab(bow):
    from openvslam_amd import synth
    tree = synth.synth_vocabulary(10, 4)
    return tree, bow.vocabulary(tree)


def _check_queries(db, ref, vecs, cov):
    for qry in sorted(vecs):
        assert same(db.score_all(vecs[qry]), ref.score_all(vecs[qry]))
        connected = cov(qry)
        min_score = min([bowdb_ref.f32(bowdb_ref.score(vecs[qry], vecs[k])[0]) for k in connected] or [0.0])
        want = ref.acquire_loop_candidates(qry, vecs[qry], connected, cov, min_score)
        assert db.acquire_loop_candidates(qry, vecs[qry], connected, cov, min_score) == want
        want = ref.acquire_relocalization_candidates(vecs[qry], cov)
        assert db.acquire_relocalization_candidates(vecs[qry], cov) == want and want


def test_end_to_end_from_descriptors(bow, vocab):
    tree, voc = vocab
    descs = _place_descriptors(tree)
    vecs = {kid: voc.transform(d)[0] for kid, d in descs.items()}
    assert all(len(v) > 50 for v in vecs.values())
    db, ref = bow.bow_database(len(vecs)), bowdb_ref.bow_database()
    for kid in sorted(vecs):
        db.add_keyframe(kid, vecs[kid])
        ref.add_keyframe(kid, vecs[kid])
    cov = lambda k: [n for n in sorted(vecs) if n != k and n // 4 == k // 4 and abs(n - k) == 1]
    _check_queries(db, ref, vecs, cov)
    # keyframes of the query's place score above the others
    sc = {k: s for k, _, s in db.score_all(vecs[0])}
    assert min(sc[k] for k in (1, 2, 3)) > max(sc[k] for k in range(4, 12))


def test_end_to_end_from_a_saved_map(bow, vocab, tmp_path):
    from openvslam_amd import io, synth
    tree, voc = vocab
    mdb, _ = synth.synth_map(n_pose=8, n_pt=300, obs_per_pose=120, seed=3)
    descs = _place_descriptors(tree, n_places=2, per_place=4, n_desc=150, seed=9)
    for kid, kf in mdb.keyframes.items():          # two places' descriptors instead of synth_map's random ones
        kf.descs = np.ascontiguousarray(descs[kid][:len(kf.keypts)])
        assert len(kf.descs) == len(kf.keypts)
    io.save_map_database(tmp_path / "map.msg", mdb)
    loaded = io.load_map_database(tmp_path / "map.msg")
    db = io.bow_database_of(loaded, voc)
    cov = io.top_covisibilities_of(loaded)
    assert len(db) == 8 and all(len(cov(k)) <= 10 for k in loaded.keyframes)
    vecs = {kid: voc.transform(loaded.keyframes[kid].descs)[0] for kid in loaded.keyframes}
    ref = bowdb_ref.bow_database()
    for kid in sorted(vecs):
        ref.add_keyframe(kid, vecs[kid])
    _check_queries(db, ref, vecs, cov)


# ---- error contract
def test_error_contract_leaves_the_handle_usable(bow):
    from openvslam_amd import _lib
    L = _lib.lib()
    db = bow.bow_database(3, max_words=8)
    ref = bowdb_ref.bow_database()
    v1, v2 = {1: .5, 4: .25, 9: .25}, {4: .5, 9: .5}
    db.add_keyframe(1, v1), ref.add_keyframe(1, v1)
    db.add_keyframe(2, v2), ref.add_keyframe(2, v2)
    q = {1: .25, 4: .25, 7: .5}
    ok = lambda: same(db.score_all(q), ref.score_all(q)) and db.query(q) == ref.query(q) and len(db) == len(ref)
    assert ok()

    def arr(ids, vals):
        return np.array(ids, np.int32), np.array(vals, np.float64)

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    out_i, out_n, out_s = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8)
    n, mc = C.c_int32(-7), C.c_int32(-7)
    INVALID, CAPACITY = -1, -4
    bad_vectors = [([3, 2], [.5, .5]), ([2, 2], [.5, .5]), ([-1, 2], [.5, .5]), ([1, 2], [.5, float("nan")]), ([1, 2], [float("inf"), .5])]
    for ids, vals in bad_vectors:
        i, v = arr(ids, vals)
        assert L.ovs_bowdb_add(db._h, 50, p(i), p(v), len(i)) == INVALID
        assert L.ovs_bowdb_query(db._h, p(i), p(v), len(i), None, 0, p(out_i), p(out_n), p(out_s), 8, C.byref(n), C.byref(mc)) == INVALID
        assert L.ovs_bowdb_score_all(db._h, p(i), p(v), len(i), p(out_i), p(out_n), p(out_s), 8, C.byref(n)) == INVALID
        assert ok()
    i, v = arr([1, 2], [.5, .5])
    assert L.ovs_bowdb_add(db._h, 1, p(i), p(v), 2) == INVALID          # the id is already present
    assert L.ovs_bowdb_erase(db._h, 77) == INVALID                      # unknown id
    assert ok()
    i9, v9 = arr(list(range(9)), [1 / 9.0] * 9)
    assert L.ovs_bowdb_add(db._h, 51, p(i9), p(v9), 9) == CAPACITY      # n > max_words
    assert L.ovs_bowdb_query(db._h, p(i9), p(v9), 9, None, 0, p(out_i), p(out_n), p(out_s), 8, C.byref(n), C.byref(mc)) == CAPACITY
    assert L.ovs_bowdb_score_all(db._h, p(i9), p(v9), 9, p(out_i), p(out_n), p(out_s), 8, C.byref(n)) == CAPACITY
    assert ok()
    qi, qv = arr(sorted(q), [q[w] for w in sorted(q)])
    out_i[:] = -5
    assert L.ovs_bowdb_score_all(db._h, p(qi), p(qv), 3, p(out_i), p(out_n), p(out_s), 1, C.byref(n)) == CAPACITY   # cap below the size
    assert L.ovs_bowdb_query(db._h, p(qi), p(qv), 3, None, 0, p(out_i), p(out_n), p(out_s), 0, C.byref(n), C.byref(mc)) == CAPACITY
    assert (out_i == -5).all() and n.value == -7 and mc.value == -7     # nothing truncated, nothing written
    assert ok()
    with pytest.raises(_lib.OvsError):
        db.add_keyframe(1, v1)
    with pytest.raises(_lib.OvsError):
        db.erase_keyframe(77)
    v3 = {0: 1.0}
    db.add_keyframe(3, v3), ref.add_keyframe(3, v3)
    assert L.ovs_bowdb_add(db._h, 52, p(i), p(v), 2) == CAPACITY        # the database is full
    assert ok()
    db.erase_keyframe(2), ref.erase_keyframe(2)
    db.add_keyframe(52, v2), ref.add_keyframe(52, v2)                  # ... and takes a keyframe again once one has left
    assert ok()
    h = C.c_void_p()
    assert L.ovs_bowdb_create(0, 0, 8, C.byref(h)) == INVALID and L.ovs_bowdb_create(0, 4, 0, C.byref(h)) == INVALID
    assert L.ovs_bowdb_create(0, 4, 1 << 20, C.byref(h)) == INVALID    # a query that cannot fit a workgroup's LDS


# ---- the C++ class
def _write_scene(path, vecs, cov, qry, min_score, frame_vec):
    def vec(v):
        return struct.pack("<i", len(v)) + b"".join(struct.pack("<id", w, v[w]) for w in sorted(v))

    def ids(a):
        return struct.pack("<i", len(a)) + struct.pack("<%di" % len(a), *a)

    blob = struct.pack("<i", len(vecs))
    for kid in sorted(vecs):
        blob += struct.pack("<i", kid) + vec(vecs[kid]) + ids(cov(kid)) + ids(cov(kid))
    blob += struct.pack("<if", qry, min_score) + vec(frame_vec)
    path.write_bytes(blob)


def test_cpp_class_returns_the_reference_candidates(places, tmp_path):
    vecs, cov, _, ref = places
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "openvslam_amd", "cpp")] + (["asan"] if SUFFIX else []))
    shim = os.path.join(ROOT, "openvslam_amd", "cpp", "test_bowdb_shim" + SUFFIX)
    for place in (0, 4):
        qry, vec, connected, min_score = loop_query(vecs, cov, place)
        assert connected == cov(qry)
        frame_vec = vecs[(place + 1) % N_PLACES * PER_PLACE + 3]
        _write_scene(tmp_path / "scene.bin", vecs, cov, qry, min_score, frame_vec)
        subprocess.check_call([shim, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")])
        raw = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.int32)
        n_loop = int(raw[0])
        loop = raw[1:1 + n_loop].tolist()
        n_reloc = int(raw[1 + n_loop])
        reloc = raw[2 + n_loop:2 + n_loop + n_reloc].tolist()
        assert 2 + n_loop + n_reloc == len(raw)
        assert loop == ref.acquire_loop_candidates(qry, vec, connected, cov, min_score) and loop
        assert reloc == ref.acquire_relocalization_candidates(frame_vec, cov) and reloc
