"""k_bow_transform at its edges, exact against oracle.bow_transform (word, weight and node: np.array_equal, nothing else): the hand-built trees of
tests/bow_trees.py (tests/test_bow_trees.py shows by the oracle alone that they have the shapes and ties claimed) through both entry points,
the device entry's count clamp and untouched slots, the error contract of both entries, and the same tree loaded from the three file formats."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_trees as bt   # noqa: E402

pytestmark = pytest.mark.gpu

LEVELSUP = (0, 1, 2, 3, 4, 5, 2**31 - 1)
INVALID, CAPACITY = -1, -4
SENTINEL = -7


@pytest.fixture(scope="module")
def ragged(oracle):
    """(vocab, desc, {levelsup: oracle triple}), computed once and read-only"""
    vocab, desc, _ = bt.ragged()
    want = {ls: oracle.bow_transform(vocab, desc, ls) for ls in LEVELSUP}
    for a in list(vocab.values()) + [desc] + [x for t in want.values() for x in t]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return vocab, desc, want


def _same(got, want, n=None):
    return all(np.array_equal(g, w[:n]) for g, w in zip(got, want))


def test_ragged_descents_for_every_levelsup(ragged):
    from openvslam_amd import bow
    vocab, desc, want = ragged
    v = bow.vocabulary(vocab, max_features=len(desc))
    for ls in LEVELSUP:
        assert _same(v.transform_features(desc, ls), want[ls]), ls
    bv, fv = v.transform(desc, 2)
    wbv, wfv = bow.assemble(*want[2])
    assert bv == wbv and fv == wfv and len(wbv) > 100 and 0 in wfv and len(wfv) > 5       # root, leaves and inner nodes as feature-vector keys


@pytest.mark.parametrize("n", bt.RAGGED_PREFIXES)
def test_ragged_partial_wavefronts_and_workgroups(ragged, n):
    """n descriptors: the rows past n leave at once, inside a wavefront (n % 4), inside a workgroup (n % 16) and in a second workgroup"""
    from openvslam_amd import bow
    vocab, desc, want = ragged
    v = bow.vocabulary(vocab, max_features=65)
    for ls in (1, 2):
        assert _same(v.transform_features(desc[:n], ls), want[ls], n), (n, ls)


@pytest.mark.parametrize("name,build", bt.flat_cases(), ids=[c[0] for c in bt.flat_cases()])
def test_ties_full_distance_and_wide_nodes(oracle, name, build):
    from openvslam_amd import bow
    vocab, desc, want_word = build()
    v = bow.vocabulary(vocab, max_features=len(desc))
    for ls in (0, 1):
        want = oracle.bow_transform(vocab, desc, ls)
        assert np.array_equal(want[0], want_word)
        assert _same(v.transform_features(desc, ls), want), (name, ls)


def _dev_call(v, frames, counts, cap, levelsup):
    """frames: (B, cap, 32) uint8. Returns the three (B, cap) outputs, sentinel-filled before the launch on a stream of its own."""
    import torch
    B = len(counts)
    d_desc = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    d_cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    d_word = torch.full((B, cap), SENTINEL, dtype=torch.int32, device="cuda")
    d_wt = torch.full((B, cap), float(SENTINEL), dtype=torch.float64, device="cuda")
    d_node = torch.full((B, cap), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                     # inputs and sentinels are in place before the other stream reads them
    s = torch.cuda.Stream()
    v.transform_batch_dev(d_desc, d_cnt, d_word, d_wt, d_node, levelsup=levelsup, stream=s.cuda_stream)
    s.synchronize()
    return d_word.cpu().numpy(), d_wt.cpu().numpy(), d_node.cpu().numpy()


@pytest.mark.parametrize("cap,counts", [(21, [0, 21, 7]), (21, [-3, 40, 1]), (1, [1, 0, 5])])
def test_transform_batch_dev_clamps_counts_and_leaves_the_rest(oracle, ragged, cap, counts):
    """the device entry works on the caller's cap and buffers (the handle's own staging holds 16 features): a count above cap means cap, a
    negative count means none, and no slot at or past the count is written"""
    from openvslam_amd import bow
    vocab, desc, want = ragged
    v = bow.vocabulary(vocab, max_features=16)
    B = len(counts)
    frames = np.stack([desc[5 + b * cap:5 + (b + 1) * cap] for b in range(B)])          # off the group alignment on purpose
    word, wt, node = _dev_call(v, frames, counts, cap, 2)
    for b in range(B):
        n = min(max(counts[b], 0), cap)
        w = oracle.bow_transform(vocab, frames[b, :n], 2)
        assert np.array_equal(word[b, :n], w[0]) and np.array_equal(wt[b, :n], w[1]) and np.array_equal(node[b, :n], w[2]), (b, n)
        assert (word[b, n:] == SENTINEL).all() and (wt[b, n:] == SENTINEL).all() and (node[b, n:] == SENTINEL).all(), (b, n)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_host_entry_error_contract(ragged):
    from openvslam_amd import _lib, bow
    vocab, desc, want = ragged
    cap = 16
    v = bow.vocabulary(vocab, max_features=cap)
    L = _lib.lib()
    d = np.ascontiguousarray(desc[:cap + 1])
    word, wt, node = np.full(cap + 1, SENTINEL, np.int32), np.full(cap + 1, float(SENTINEL)), np.full(cap + 1, SENTINEL, np.int32)

    def untouched():
        return (word == SENTINEL).all() and (wt == SENTINEL).all() and (node == SENTINEL).all()

    call = lambda dd, n, ls, a, b, c: L.ovs_bow_transform(v._h, _p(dd), n, ls, _p(a), _p(b), _p(c))
    assert call(d, -1, 2, word, wt, node) == INVALID and untouched()
    assert call(d, 4, -1, word, wt, node) == INVALID and untouched()
    assert call(None, 4, 2, word, wt, node) == INVALID and untouched()
    assert call(d, 4, 2, None, wt, node) == INVALID and untouched()
    assert call(d, 4, 2, word, None, node) == INVALID and untouched()
    assert call(d, 4, 2, word, wt, None) == INVALID and untouched()
    assert L.ovs_bow_transform(None, _p(d), 4, 2, _p(word), _p(wt), _p(node)) == INVALID and untouched()
    assert call(None, 0, 2, None, None, None) == 0
    assert call(d, 0, 2, word, wt, node) == 0 and untouched()
    assert call(d, cap + 1, 2, word, wt, node) == CAPACITY and untouched()
    # the handle is still good: exactly max_features
    assert call(d, cap, 2, word, wt, node) == 0
    assert _same((word[:cap], wt[:cap], node[:cap]), want[2], cap)
    assert word[cap] == SENTINEL and wt[cap] == SENTINEL and node[cap] == SENTINEL


def test_device_entry_error_contract(ragged):
    import torch
    from openvslam_amd import _lib, bow
    vocab, desc, want = ragged
    B, cap = 2, 8
    v = bow.vocabulary(vocab, max_features=16)
    L = _lib.lib()
    d_desc = torch.from_numpy(np.array(desc[:B * cap]).reshape(B, cap, 32)).cuda()
    d_cnt = torch.tensor([cap, 3], dtype=torch.int32, device="cuda")
    d_word = torch.full((B, cap), SENTINEL, dtype=torch.int32, device="cuda")
    d_wt = torch.full((B, cap), float(SENTINEL), dtype=torch.float64, device="cuda")
    d_node = torch.full((B, cap), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = dict(v=v._h, desc=d_desc.data_ptr(), cnt=d_cnt.data_ptr(), batch=B, cap=cap, ls=2, word=d_word.data_ptr(), wt=d_wt.data_ptr(),
                node=d_node.data_ptr())

    def call(**change):
        a = dict(good, **change)
        st = L.ovs_bow_transform_dev(a["v"], a["desc"], a["cnt"], a["batch"], a["cap"], a["ls"], a["word"], a["wt"], a["node"], None)
        torch.cuda.synchronize()
        return st

    def untouched():
        return bool((d_word == SENTINEL).all() and (d_wt == SENTINEL).all() and (d_node == SENTINEL).all())

    for key in ("v", "desc", "cnt", "word", "wt", "node"):
        assert call(**{key: None}) == INVALID and untouched(), key
    for change in (dict(batch=0), dict(batch=-1), dict(cap=0), dict(cap=-5), dict(ls=-1)):
        assert call(**change) == INVALID and untouched(), change
    assert call() == 0
    word, wt, node = d_word.cpu().numpy(), d_wt.cpu().numpy(), d_node.cpu().numpy()
    for b, n in enumerate((cap, 3)):
        sl = slice(b * cap, b * cap + n)
        assert np.array_equal(word[b, :n], want[2][0][sl]) and np.array_equal(wt[b, :n], want[2][1][sl]) and np.array_equal(node[b, :n], want[2][2][sl])
        assert (word[b, n:] == SENTINEL).all() and (wt[b, n:] == SENTINEL).all() and (node[b, n:] == SENTINEL).all()


@pytest.mark.parametrize("fmt", ["text", "dbow2", "fbow"])
def test_loaded_ragged_vocabulary_transforms_like_the_source_tree(oracle, ragged, tmp_path, fmt):
    """An FBoW file carries no depth: the loaded tree's is the deepest node's level (3), so there the source tree is asked at that depth."""
    import vocab_io
    from openvslam_amd import bow
    vocab, desc, want = ragged
    path = tmp_path / ("orb_vocab." + fmt)
    vocab_io.WRITERS[fmt](str(path), vocab)
    voc = bow.load_vocabulary(path, max_features=len(desc))
    src = dict(vocab, weight=vocab["weight"].astype(np.float32).astype(np.float64), depth=bt.depth_on_disk(vocab, fmt))
    assert voc.depth == src["depth"]
    order = vocab_io.fbow_node_order(vocab) if fmt == "fbow" else np.arange(len(vocab["word_id"]))      # loaded numbering -> source node
    for ls in (0, 1, 2, 3, 4):
        word, weight, node = voc.transform_features(desc, ls)
        w = want[ls] if src["depth"] == vocab["depth"] else oracle.bow_transform(src, desc, ls)
        assert np.array_equal(word, w[0]) and np.array_equal(weight, w[1]) and np.array_equal(order[node], w[2]), (fmt, ls)
