"""The all-pairs Hamming stage on FP4 matrix instructions (k_hamming_near): constructed problems for what that form could get wrong --
a bit position dropped, doubled or paired with the wrong partner along K, operand roles or rows / columns swapped, tile and
workgroup edges, the queue / drain path. Every case goes through match.robust and is compared exactly with the CPU oracle and with the
popcount form of the stage."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def match():
    from openvslam_amd import match
    return match


def _flip(desc, bits):
    b = np.unpackbits(desc)
    b[np.asarray(bits, dtype=np.int64)] ^= 1
    return np.packbits(b)


def _check(match, oracle, d1, d2, ratio, cap1, cap2, valid=None):
    """matrix == popcount == oracle, pair by pair; returns the oracle's pairs"""
    want = oracle.robust_brute_force_match(d1, d2, valid, ratio)
    for path in ("matrix", "popcount"):
        m = match.robust(ratio, False, max_n1=cap1, max_n2=cap2, near_path=path)
        got = m.brute_force_match(d1, d2, valid)
        assert np.array_equal(got, want), (path, ratio, len(d1), len(d2))
    return want


def bit_position_problem(seed=7):
    """512 frame and 512 keyframe descriptors. Keyframe 2k is frame perm[2k] with exactly 50 bits flipped, keyframe 2k + 1 is frame
    perm[2k + 1] with exactly 51 flipped, bit k among them in both (k = 0..255). THR_LOW is 50: the 50s match, the 51s do not, and a
    bit that the kernel drops, doubles or pairs with the wrong partner moves one of the two by 1 or 2 and flips its outcome."""
    rng = np.random.default_rng(seed)
    frame = rng.integers(0, 256, size=(512, 32), dtype=np.uint8)
    perm = rng.permutation(512)
    key = np.empty_like(frame)
    for k in range(256):
        others = np.array([b for b in rng.permutation(256) if b != k])
        key[2 * k] = _flip(frame[perm[2 * k]], [k, *others[:49]])
        key[2 * k + 1] = _flip(frame[perm[2 * k + 1]], [k, *others[:50]])
    return frame, key, perm


@pytest.mark.parametrize("ratio", [0.9, 0.6])
def test_every_bit_position_decides_once(match, oracle, ratio):
    frame, key, perm = bit_position_problem()
    want = _check(match, oracle, frame, key, ratio, 512, 512)
    # the construction itself: the oracle accepts exactly the 256 even keyframes, each with its own frame descriptor
    assert np.array_equal(want[:, 1], np.arange(0, 512, 2)) and np.array_equal(want[:, 0], perm[0:512:2])


def _problem(rng, n1, n2, frac=0.6):
    """n1 frame / n2 keyframe descriptors; a fraction of the smaller side are copies with 0..60 flipped bits (both sides of THR_LOW and
    of the near bounds); the LAST frame descriptor always has a partner three bits away, so the last row of a partial tile is matched"""
    d1 = rng.integers(0, 256, size=(n1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, size=(n2, 32), dtype=np.uint8)
    n_true = max(1, int(min(n1, n2) * frac))
    src = rng.permutation(n1)[:n_true]
    src[0] = n1 - 1
    dst = rng.permutation(n2)[:n_true]
    for i, (s, t) in enumerate(zip(src, dst)):
        d2[t] = _flip(d1[s], rng.permutation(256)[:3 if i == 0 else int(rng.integers(0, 61))])
    return d1, d2


def test_asymmetric_sizes_and_permutations(match, oracle):
    """n1 = 130, n2 = 600: five frame tiles against three query chunks (three different rotated start tiles); with different sizes and
    permutations on the two sides, swapped rows / columns or operand roles cannot pass"""
    rng = np.random.default_rng(21)
    d1, d2 = _problem(rng, 130, 600, frac=0.9)
    for ratio in (0.9, 0.6):
        want = _check(match, oracle, d1, d2, ratio, 256, 1024)
        assert len(want) > 30


@pytest.mark.parametrize("n1", [1, 31, 32, 33, 95, 96, 97, 127, 128, 129, 160])
def test_tile_and_workgroup_edges(match, oracle, n1):
    rng = np.random.default_rng(300 + n1)
    for n2 in (1, 255, 256, 257):
        d1, d2 = _problem(rng, n1, n2)
        want = _check(match, oracle, d1, d2, 0.9, 256, 512)
        assert n1 - 1 in want[:, 0]


def test_batched_call_mixing_edge_sizes(match, oracle):
    import torch
    rng = np.random.default_rng(41)
    sizes = [(1, 1), (31, 255), (32, 256), (33, 257), (95, 1), (96, 255), (97, 256), (127, 257), (128, 255), (129, 256), (160, 257),
             (0, 200), (150, 0)]
    B, cap1, cap2 = len(sizes), 256, 512
    d1 = np.zeros((B, cap1, 32), np.uint8)
    d2 = np.zeros((B, cap2, 32), np.uint8)
    for b, (a, c) in enumerate(sizes):
        if a and c:
            d1[b, :a], d2[b, :c] = _problem(rng, a, c)
        else:   # an empty side: the other side's descriptors are all equal, so anything matched by mistake would be accepted
            d1[b], d2[b] = 0x5A, 0x5A
    n1 = np.array([s[0] for s in sizes], np.int32)
    n2 = np.array([s[1] for s in sizes], np.int32)
    out = {}
    for path in ("matrix", "popcount"):
        m = match.robust(0.9, False, max_n1=cap1, max_n2=cap2, max_batch=B, near_path=path)
        pairs = torch.full((B, cap2, 2), -1, dtype=torch.int32, device="cuda")
        cnt = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        m.brute_force_match_batch_dev(torch.from_numpy(d1).cuda(), torch.from_numpy(n1).cuda(), torch.from_numpy(d2).cuda(),
                                      torch.from_numpy(n2).cuda(), pairs, cnt, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out[path] = (pairs.cpu().numpy(), cnt.cpu().numpy())
    for b, (a, c) in enumerate(sizes):
        want = oracle.robust_brute_force_match(d1[b, :a], d2[b, :c], None, 0.9) if a and c else np.zeros((0, 2), np.int32)
        for path in ("matrix", "popcount"):
            pairs, cnt = out[path]
            assert cnt[b] == len(want) and np.array_equal(pairs[b, :cnt[b]], want), (path, a, c)


def queue_problem(seed=5):
    """128 queries with 40 near candidates each (below the 64-entry list segment: the normal path, not the overflow fall-back): query q
    has 40 frame descriptors of its own at 5..44 flipped bits, 5120 frame descriptors in all. A wave queues 64 x 40 tile columns, so its
    128-slot ring is drained in full many times, wraps around and ends on a partial drain."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 256, size=(128, 32), dtype=np.uint8)
    frame = np.empty((128 * 40, 32), np.uint8)
    order = rng.permutation(128 * 40)
    for q in range(128):
        for i in range(40):
            frame[order[q * 40 + i]] = _flip(key[q], rng.permutation(256)[:5 + i])
    return frame, key


def test_queue_wraps_and_drains(match, oracle):
    frame, key = queue_problem()
    want = _check(match, oracle, frame, key, 0.9, 5120, 128)
    assert len(want) > 60
    valid = (np.arange(128) % 3 != 0).astype(np.uint8)   # every third query inactive
    want_v = _check(match, oracle, frame, key, 0.9, 5120, 128, valid=valid)
    assert 0 < len(want_v) < len(want) and valid[want_v[:, 1]].all()
