"""GPU parity: HIP robust::brute_force_match / best2 (through the C ABI) == CPU oracle, exactly (match pairs and order)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def match():
    from openvslam_amd import match
    return match


def _descs(rng, n1, n2, n_true, max_flip=40):
    """n2 keyframe descriptors; n_true of the n1 frame descriptors are bit-flipped copies (random pairs sit
    at ~128+-8 and never pass THR_LOW, so matches must be constructed)."""
    d2 = rng.integers(0, 256, size=(n2, 32), dtype=np.uint8)
    d1 = rng.integers(0, 256, size=(n1, 32), dtype=np.uint8)
    src = rng.permutation(n2)[:n_true]
    dst = rng.permutation(n1)[:n_true]
    for s, t in zip(src, dst):
        bits = np.unpackbits(d2[s])
        k = int(rng.integers(0, max_flip + 1))
        flip = rng.permutation(256)[:k]
        bits[flip] ^= 1
        d1[t] = np.packbits(bits)
    return d1, d2


@pytest.fixture(params=["matrix", "popcount"])
def near_path(request):
    """Both implementations of the all-pairs stage (ovs_matcher_set_near_path) run every brute_force_match test."""
    return request.param


@pytest.mark.parametrize("n1,n2,n_true", [(2000, 2000, 1200), (2004, 1987, 1500), (1, 1, 1), (300, 5, 5), (5, 300, 5), (777, 1023, 0)])
@pytest.mark.parametrize("ratio", [0.9, 0.6])
def test_brute_force_match(match, oracle, n1, n2, n_true, ratio, near_path):
    rng = np.random.default_rng(n1 * 31 + n2)
    d1, d2 = _descs(rng, n1, n2, min(n_true, n1, n2))
    valid = (rng.random(n2) < 0.9).astype(np.uint8)
    m = match.robust(ratio, False, max_n1=2048, max_n2=2048, near_path=near_path)
    for v in (None, valid):
        want = oracle.robust_brute_force_match(d1, d2, v, ratio)
        got = m.brute_force_match(d1, d2, v)
        assert np.array_equal(got, want)
    # optional frame-side mask: a third of the frame keypoints (true matches among them) must never be matched or block the ratio test
    v1 = (rng.random(n1) < 0.67).astype(np.uint8)
    want1 = oracle.robust_brute_force_match(d1, d2, valid, ratio, frm_valid=v1)
    got1 = m.brute_force_match(d1, d2, valid, frm_valid=v1)
    assert np.array_equal(got1, want1) and (len(want1) == 0 or v1[want1[:, 0]].all())
    if n_true >= 1000:
        assert len(want) > n_true // 3 and 0 < len(want1) < len(want)


# Handle capacities of the resolver's two forms (tests/test_match_bf_plan.py holds the table): the four-wave form with every query's counts and top-8
# staged in LDS, and the one-wave form that reads them from memory -- the one the C++ class layer's 4096 x 4096 handles run
ONE_WAVE = dict(max_n1=2048, max_n2=4096)


@pytest.mark.parametrize("caps", [dict(max_n1=256, max_n2=256), ONE_WAVE], ids=["staged", "one_wave"])
def test_claim_conflicts(match, oracle, near_path, caps):
    """Several keyframe descriptors compete for the same frame descriptor: exercises the already-matched rule."""
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, size=(40, 32), dtype=np.uint8)
    d1 = np.repeat(base, 3, axis=0)     # 120 frame descriptors, triplets of near-duplicates
    d2 = np.repeat(base, 5, axis=0)     # 200 keyframe descriptors, 5 claimants per triplet
    for d in (d1, d2):
        for i in range(len(d)):
            bits = np.unpackbits(d[i])
            bits[rng.permutation(256)[:int(rng.integers(0, 12))]] ^= 1
            d[i] = np.packbits(bits)
    for ratio in (0.6, 0.9, 1.0):
        m = match.robust(ratio, False, near_path=near_path, **caps)
        assert np.array_equal(m.brute_force_match(d1, d2), oracle.robust_brute_force_match(d1, d2, None, ratio))
        v1 = (np.arange(len(d1)) % 3 != 0).astype(np.uint8)   # the first of every triplet is masked: claimants fall through to the next
        assert np.array_equal(m.brute_force_match(d1, d2, frm_valid=v1), oracle.robust_brute_force_match(d1, d2, None, ratio, frm_valid=v1))


@pytest.mark.parametrize("caps", [dict(max_n1=128, max_n2=128), ONE_WAVE], ids=["staged", "one_wave"])
def test_overflowing_near_lists_fall_back_exactly(match, oracle, near_path, caps):
    """Many identical descriptors overflow the near lists -> literal serial replay path."""
    d1 = np.zeros((100, 32), np.uint8)
    d2 = np.zeros((60, 32), np.uint8)
    d1[::7, 0] = 1
    d2[::5, 3] = 0x80
    for ratio in (0.6, 0.9):
        m = match.robust(ratio, False, near_path=near_path, **caps)
        assert np.array_equal(m.brute_force_match(d1, d2), oracle.robust_brute_force_match(d1, d2, None, ratio))
        v1 = (np.arange(len(d1)) % 3 != 0).astype(np.uint8)   # the first of every triplet is masked: claimants fall through to the next
        assert np.array_equal(m.brute_force_match(d1, d2, frm_valid=v1), oracle.robust_brute_force_match(d1, d2, None, ratio, frm_valid=v1))
    # ratio 1.01: duplicates are accepted one by one until the frame side runs out
    m = match.robust(1.01, False, near_path=near_path, **caps)
    got = m.brute_force_match(d1, d2)
    want = oracle.robust_brute_force_match(d1, d2, None, 1.01)
    assert np.array_equal(got, want) and len(want) > 10


@pytest.mark.parametrize("caps", [dict(max_n1=128, max_n2=128), ONE_WAVE], ids=["staged", "one_wave"])
def test_dry_top8_rescans_the_near_list(match, oracle, near_path, caps):
    """24 frame and 24 keyframe descriptors, all within 4 bits of one base descriptor: every query's near list names all 24 frame descriptors, none
    overflows. From the ninth query on the eight keys held in registers are all claimed while the list is longer, so the resolver rescans the whole
    list (and refills the registers). At ratio 1.01 every query accepts as long as an unclaimed frame descriptor is left (best <= 50, second >= best):
    24 pairs by the oracle alone."""
    rng = np.random.default_rng(24)
    base = np.unpackbits(rng.integers(0, 256, size=32, dtype=np.uint8))

    def near_copies(n):
        out = np.empty((n, 32), np.uint8)
        for i in range(n):
            bits = base.copy()
            bits[rng.permutation(256)[:int(rng.integers(0, 5))]] ^= 1
            out[i] = np.packbits(bits)
        return out

    d1, d2 = near_copies(24), near_copies(24)
    for ratio in (1.01, 0.9):
        want = oracle.robust_brute_force_match(d1, d2, None, ratio)
        if ratio == 1.01:
            assert len(want) == 24
        m = match.robust(ratio, False, near_path=near_path, **caps)
        assert np.array_equal(m.brute_force_match(d1, d2), want), ratio


def test_a_smaller_handle_leaves_a_larger_ones_launches_valid(match, oracle):
    """Both handles need more dynamic LDS than a kernel gets by default (123008 and 83968 bytes of the same resolver form); the limit is a property of
    the kernel, not of the handle, and the second create must not lower what the first one raised."""
    rng = np.random.default_rng(70)
    d1, d2 = _descs(rng, 70, 70, 50)
    want = oracle.robust_brute_force_match(d1, d2, None, 0.9)
    large = match.robust(0.9, False, max_n1=3000, max_n2=3000)
    small = match.robust(0.9, False, max_n1=2048, max_n2=2048)
    assert len(want) > 10
    assert np.array_equal(small.brute_force_match(d1, d2), want)
    assert np.array_equal(large.brute_force_match(d1, d2), want)


def test_best2_and_distance_identities(match, oracle):
    rng = np.random.default_rng(9)
    q, t = _descs(rng, 500, 700, 300)
    ctx = match._matcher_ctx(max_n1=1024, max_n2=1024)
    valid = (rng.random(700) < 0.8).astype(np.uint8)
    for v in (None, valid):
        gi, gb, gs = match.hamming_best2(ctx, q, t, v)
        wi, wb, ws = oracle.hamming_best2(q, t, v)
        assert np.array_equal(gi, wi) and np.array_equal(gb, wb) and np.array_equal(gs, ws)
    # d(a,a)=0 and d(a,~a)=256 through the kernel
    a = rng.integers(0, 256, size=(4, 32), dtype=np.uint8)
    gi, gb, gs = match.hamming_best2(ctx, a, a)
    assert np.array_equal(gb, np.zeros(4)) and np.array_equal(gi, np.arange(4))
    gi, gb, gs = match.hamming_best2(ctx, a[:1], ~a[:1])
    assert gb[0] == 256 and gi[0] == -1   # strict '<' against MAX_HAMMING_DIST: 256 never wins


def test_batch_dev(match, oracle, near_path):
    import torch
    rng = np.random.default_rng(11)
    B, cap = 4, 512
    d1 = np.zeros((B, cap, 32), np.uint8)
    d2 = np.zeros((B, cap, 32), np.uint8)
    n1 = np.array([500, 512, 37, 400], np.int32)
    n2 = np.array([480, 512, 300, 1], np.int32)
    for b in range(B):
        a, c = _descs(rng, n1[b], n2[b], min(n1[b], n2[b]) // 2)
        d1[b, :n1[b]] = a
        d2[b, :n2[b]] = c
    m = match.robust(0.9, False, max_n1=cap, max_n2=cap, max_batch=B, near_path=near_path)
    td1, td2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    tn1, tn2 = torch.from_numpy(n1).cuda(), torch.from_numpy(n2).cuda()
    pairs = torch.zeros((B, cap, 2), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((B,), dtype=torch.int32, device="cuda")
    m.brute_force_match_batch_dev(td1, tn1, td2, tn2, pairs, cnt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for b in range(B):
        want = oracle.robust_brute_force_match(d1[b, :n1[b]], d2[b, :n2[b]], None, 0.9)
        got = pairs[b, :int(cnt[b])].cpu().numpy()
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n1", [1, 31, 32, 33, 65, 255, 257])
def test_near_stage_edge_patterns(match, oracle, near_path, n1):
    """Descriptors the all-pairs stage could get wrong: all-zero / all-one descriptors on either side (the matrix path's acceptance
    bound |b| - near_thr goes negative, a padded tile row would then look near), exact duplicates of the LAST frame descriptor (the one
    the matrix path re-reads for rows past n1), a keyframe-side count that leaves partial 32-query tiles and partial workgroups."""
    rng = np.random.default_rng(100 + n1)
    for n2 in (1, 33, 300):
        d1 = rng.integers(0, 256, size=(n1, 32), dtype=np.uint8)
        d2 = rng.integers(0, 256, size=(n2, 32), dtype=np.uint8)
        d1[0] = 0
        d1[-1] = rng.integers(0, 2, size=32, dtype=np.uint8)        # very few bits set
        d2[0] = 0
        d2[n2 // 2] = 255
        d2[-1] = d1[-1]                                             # exact copy of the last frame descriptor
        if n2 > 4:
            d2[3] = d1[-1] ^ np.eye(32, dtype=np.uint8)[5]          # one bit away from it
            d2[4] = np.eye(32, dtype=np.uint8)[7] * 3               # two bits set: near the all-zero frame descriptor
        if n1 > 2:
            d1[1] = 255
        for ratio in (0.9, 0.6, 1.01):
            m = match.robust(ratio, False, max_n1=512, max_n2=512, near_path=near_path)
            want = oracle.robust_brute_force_match(d1, d2, None, ratio)
            got = m.brute_force_match(d1, d2, None)
            assert np.array_equal(got, want), (n1, n2, ratio)


def test_near_paths_agree_on_large_batch(match):
    """Full-size property (no oracle: 64 problems of ~2000 x 2000): the matrix path and the popcount path return the same pairs."""
    import torch
    rng = np.random.default_rng(9)
    B, cap = 64, 2048
    n1 = rng.integers(1900, 2049, B).astype(np.int32)
    n2 = rng.integers(1900, 2049, B).astype(np.int32)
    d2 = rng.integers(0, 256, size=(B, cap, 32), dtype=np.uint8)
    d1 = d2[:, ::-1].copy()
    noise = (rng.random((B, cap, 32)) < 0.02).astype(np.uint8) * rng.integers(1, 256, size=(B, cap, 32), dtype=np.uint8)
    d1 ^= noise                                                     # ~5 flipped bits per descriptor: most pairs are true matches
    d1[:, 100:140] = d1[:, 100:101]                                 # a cluster of duplicates: claim conflicts and long near lists
    td1, td2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    tn1, tn2 = torch.from_numpy(n1).cuda(), torch.from_numpy(n2).cuda()
    out = {}
    for path in ("matrix", "popcount"):
        m = match.robust(0.9, False, max_n1=cap, max_n2=cap, max_batch=B, near_path=path)
        pairs = torch.zeros((B, cap, 2), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((B,), dtype=torch.int32, device="cuda")
        m.brute_force_match_batch_dev(td1, tn1, td2, tn2, pairs, cnt, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out[path] = (pairs.cpu().numpy(), cnt.cpu().numpy())
    assert np.array_equal(out["matrix"][1], out["popcount"][1]) and out["matrix"][1].min() > 1000
    for b in range(B):
        k = out["matrix"][1][b]
        assert np.array_equal(out["matrix"][0][b, :k], out["popcount"][0][b, :k])


def test_full_size_batch_against_the_oracle(match, oracle, near_path):
    """The regime bench.py times: one launch over 64 problems of ~2000 x 2000 (cap 2048). 16 of the 64 problems (every fourth) are compared
    with the CPU oracle pair by pair; duplicates clusters and heavy-noise rows keep the claim resolver and the ratio test busy."""
    import torch
    rng = np.random.default_rng(19)
    B, cap = 64, 2048
    n1 = rng.integers(1900, 2049, B).astype(np.int32)
    n2 = rng.integers(1900, 2049, B).astype(np.int32)
    n1[0] = n2[0] = cap
    d2 = rng.integers(0, 256, size=(B, cap, 32), dtype=np.uint8)
    d1 = d2[:, rng.permutation(cap)].copy()
    d1 ^= (rng.random((B, cap, 32)) < 0.03).astype(np.uint8) * rng.integers(1, 256, size=(B, cap, 32), dtype=np.uint8)
    d1[:, 100:140] = d1[:, 100:101]                                 # duplicates: several frame descriptors claim one keyframe descriptor
    d2[:, 500:520] = d2[:, 500:501]                                 # and the other way round: best == second best, the ratio test rejects
    d1[:, 900:1000] ^= (rng.random((B, 100, 32)) < 0.25).astype(np.uint8) * rng.integers(1, 256, size=(B, 100, 32), dtype=np.uint8)  # around THR_LOW
    td1, td2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    tn1, tn2 = torch.from_numpy(n1).cuda(), torch.from_numpy(n2).cuda()
    m = match.robust(0.9, False, max_n1=cap, max_n2=cap, max_batch=B, near_path=near_path)
    pairs = torch.zeros((B, cap, 2), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((B,), dtype=torch.int32, device="cuda")
    m.brute_force_match_batch_dev(td1, tn1, td2, tn2, pairs, cnt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pairs, cnt = pairs.cpu().numpy(), cnt.cpu().numpy()
    for b in range(0, B, 4):
        want = oracle.robust_brute_force_match(d1[b, :n1[b]], d2[b, :n2[b]], None, 0.9)
        assert len(want) > 1000
        assert cnt[b] == len(want) and np.array_equal(pairs[b, :cnt[b]], want), b
