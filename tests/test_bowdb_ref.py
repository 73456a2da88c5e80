"""The reference of the BoW database tests (tests/bowdb_ref.py) against hand-worked cases of DESIGN.md 3.8 rules 1, 3, 5 and 6, and
the "places" scenes test_gpu_bowdb.py runs on the device: on the reference alone, a loop query from every place returns keyframes of that
place only and every gate drops something. No device."""
import random

import bowdb_ref


def test_score_hand_worked_dyadic():
    q = {1: .5, 2: .25, 7: .25}
    k = {2: .5, 7: .25, 9: .25}
    # word 2: |.25 - .5| - .25 - .5 = -.5; word 7: |0| - .25 - .25 = -.5; s = -1 -> score .5
    assert bowdb_ref.score(q, k) == (0.5, 2)
    assert bowdb_ref.score(k, q) == (0.5, 2)
    sc, n = bowdb_ref.score(q, {3: 1.0})
    assert n == 0 and sc == 0.0 and str(sc) == "0.0"      # +0.0, not -0.0
    assert bowdb_ref.score(q, {}) == (0.0, 0) and bowdb_ref.score({}, k) == (0.0, 0)
    assert bowdb_ref.score(q, q) == (1.0, 3)               # an L1-normalised vector against itself


def test_f32_narrowing():
    assert bowdb_ref.f32(0.8) == 0.800000011920928955078125 and bowdb_ref.f32(0.5) == 0.5


Q5 = {w: .2 for w in (1, 2, 3, 4, 5)}


def test_rule3_exactly_on_the_gate_is_dropped():
    """max_common 5: 0.8f * 5.0f rounds to 4.0f, and 4.0f > 4.0f is false."""
    db = bowdb_ref.bow_database()
    db.add_keyframe(10, Q5)
    db.add_keyframe(11, {1: .2, 2: .2, 3: .2, 4: .2, 9: .2})     # 4 common words: exactly on the gate
    db.add_keyframe(12, {1: .1, 2: .1, 3: .2, 4: .2, 5: .4})
    db.add_keyframe(13, {8: 1.0})                                 # no common word: not even an initial candidate
    surv, max_common = db.query(Q5)
    assert max_common == 5 and [s[0] for s in surv] == [10, 12] and [s[1] for s in surv] == [5, 5]
    # with the holders of the maximum rejected the gate comes from the remaining maximum: 4 > 0.8f * 4 = 3.2
    surv, max_common = db.query(Q5, reject=[10, 12])
    assert max_common == 4 and [s[0] for s in surv] == [11]
    assert db.query({77: 1.0}) == ([], 0)


Q4 = {1: .25, 2: .25, 3: .25, 4: .25}
A, C, R = 20, 21, 22


def _rule5_db():
    db = bowdb_ref.bow_database()
    db.add_keyframe(A, Q4)                                           # score 1.0
    db.add_keyframe(C, {1: .25, 2: .25, 3: .25, 4: .125, 9: .125})   # terms -.5 -.5 -.5 -.25 -> score .875
    db.add_keyframe(R, Q4)                                           # score 1.0, but connected to the query: rejected
    return db


def test_rule5_a_neighbour_outside_the_candidates_is_skipped():
    db = _rule5_db()
    assert [(k, n, s) for k, n, s in db.score_all(Q4)] == [(A, 4, 1.0), (C, 4, .875), (R, 4, 1.0)]
    cov = {A: [], C: [R]}
    # R skipped: totals 1.0 (A) and .875 (C), gate .75 -> both. Were R counted, C's record would be (1.875, R) and A's 1.0 would fall.
    assert db.acquire_loop_candidates(99, Q4, [R], lambda k: cov[k], 0.0) == [A, C]
    # as a relocalisation query nothing is rejected: C's record is (1.875, R), R's own (1.0, R), A's (1.0, A): the gate 1.40625 keeps one
    cov[R] = []
    assert db.acquire_relocalization_candidates(Q4, lambda k: cov[k]) == [R]
    # rule 4: C's .875 is below min_score .9 -> A alone
    assert db.acquire_loop_candidates(99, Q4, [R], lambda k: cov[k], 0.9) == [A]


def test_rule6_a_duplicate_best_is_returned_once():
    db = _rule5_db()
    cov = {A: [C], C: [A]}
    trace = {}
    # both records total 1.875 with best = A
    assert db.acquire_loop_candidates(99, Q4, [R], lambda k: cov[k], 0.0, trace) == [A]
    assert trace["dropped_gate6"] == []
    cov = {A: [], C: [A]}
    # A's record (1.0, A) is below .75 * 1.875; C's (1.875, A) stays
    assert db.acquire_loop_candidates(99, Q4, [R], lambda k: cov[k], 0.0, trace) == [A]
    assert trace["dropped_gate6"] == [A]


# ---- the "places" scenes (test_gpu_bowdb.py runs the same ones on the device)
N_WORDS, N_PLACES, POOL, PER_PLACE, FROM_POOL, FROM_ANYWHERE = 4096, 6, 300, 8, 200, 40
PLACES_SEED = 542   # gates 4 and 6 each drop something in about half of the places of a random scene; this seed does in all six


def places_scene(seed=PLACES_SEED):
    """{keyframe id: bow_vec} of N_PLACES x PER_PLACE keyframes (id // PER_PLACE = place), and the covisibility callable: a keyframe
    sees the keyframes of its place at most two ids away, nearer first, lower id first."""
    rng = random.Random(seed)
    vecs = {}
    for place in range(N_PLACES):
        pool = rng.sample(range(N_WORDS), POOL)
        for j in range(PER_PLACE):
            words = sorted(set(rng.sample(pool, FROM_POOL)) | set(rng.sample(range(N_WORDS), FROM_ANYWHERE)))
            weights = [rng.uniform(0.5, 9.0) for _ in words]
            norm = 0.0
            for w in weights:     # L1 norm in ascending word order, as DBoW2 normalises a std::map
                norm += abs(w)
            vecs[place * PER_PLACE + j] = {w: v / norm for w, v in zip(words, weights)}

    def covisibilities(kid):
        place = kid // PER_PLACE
        near = [k for k in range(place * PER_PLACE, (place + 1) * PER_PLACE) if k != kid and abs(k - kid) <= 2]
        return sorted(near, key=lambda k: (abs(k - kid), k))

    return vecs, covisibilities


def loop_query(vecs, covisibilities, place):
    """The loop detector's call for the first keyframe of a place: (query id, its vector, connected ids, min_score), min_score being the
    lowest score of the query against its connected keyframes, as upstream's loop_detector computes it."""
    qry = place * PER_PLACE
    connected = covisibilities(qry)
    min_score = min(bowdb_ref.f32(bowdb_ref.score(vecs[qry], vecs[k])[0]) for k in connected)
    return qry, vecs[qry], connected, min_score


def test_places_scenes_exercise_every_gate():
    vecs, cov = places_scene()
    db = bowdb_ref.bow_database()
    for kid in sorted(vecs):
        db.add_keyframe(kid, vecs[kid])
    assert len(db) == N_PLACES * PER_PLACE
    for place in range(N_PLACES):
        qry, vec, connected, min_score = loop_query(vecs, cov, place)
        trace = {}
        got = db.acquire_loop_candidates(qry, vec, connected, cov, min_score, trace)
        print(place, got, {k: len(v) for k, v in trace.items()})
        assert got and all(k // PER_PLACE == place for k in got)
        assert qry not in got and not set(connected) & set(got)
        assert trace["dropped_gate3"] and trace["dropped_gate4"] and trace["dropped_gate6"]
        reloc = db.acquire_relocalization_candidates(vec, cov)
        assert reloc and all(k // PER_PLACE == place for k in reloc)
