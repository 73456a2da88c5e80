"""The BoW transform's edge inputs (tests/bow_trees.py) held against the oracle alone: the trees and queries really have the shapes, ties and
shallow leaves the device tests (tests/test_gpu_bow_edges.py) rely on; the second restatement of rule 29 equals the oracle on all of them; and
ovs_vocab_create refuses a child list that is not a tree before it touches a device. No test here launches anything."""
import ctypes as C

import numpy as np
import pytest

import bow_trees as bt
import nversion_numpy as nv

LEVELSUP = (0, 1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def ragged():
    vocab, desc, want = bt.ragged()
    for a in list(vocab.values()) + [desc, want]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return vocab, desc, want


def test_ragged_has_the_stated_shape(ragged):
    vocab, desc, _ = ragged
    level, parent = bt.levels(vocab)
    fan = np.diff(vocab["child_start"])
    leaf = vocab["word_id"] >= 0
    assert vocab["depth"] == 4 and level[leaf].max() == 3 and len(desc) == 256
    assert fan[0] == 3 and np.array_equal(np.flatnonzero(level == 1), [1, 2, 3])
    a, b, c = 1, 2, 3
    assert leaf[a] and fan[b] == 1 and fan[c] == 16
    b1 = int(vocab["children"][vocab["child_start"][b]])
    assert fan[b1] == 17
    c_kids = vocab["children"][vocab["child_start"][c]:vocab["child_start"][c + 1]]
    assert leaf[c_kids[0]] and fan[c_kids].tolist() == [0, 15, 32, 33, 31] + [0] * 11
    assert sorted(np.unique(level[leaf]).tolist()) == [1, 2, 3] and leaf.sum() == 1 + 12 + 17 + 111
    assert ((fan == 0) == leaf).all() and np.array_equal(vocab["word_id"][leaf], np.arange(leaf.sum()))
    zero = leaf & (vocab["weight"] == 0)
    assert 3 <= zero.sum() <= 20 and len(np.unique(level[zero])) >= 2          # a few weight-0 words, not all on one level
    # a child is its parent's descriptor with 40 bits flipped
    d = np.unpackbits(vocab["desc"][1:] ^ vocab["desc"][parent[1:]], axis=1).sum(1)
    assert (d == 40).all()


def test_ragged_queries_reach_every_word_unambiguously(oracle, ragged):
    vocab, desc, want = ragged
    w, wt, nd = oracle.bow_transform(vocab, desc, 0)
    assert np.array_equal(w, want) and np.array_equal(wt, vocab["weight"][vocab["word_id"] >= 0][want])
    assert np.array_equal(np.unique(w), np.arange((vocab["word_id"] >= 0).sum()))
    flips = np.unpackbits(desc ^ vocab["desc"][vocab["word_id"] >= 0][want], axis=1).sum(1)
    assert flips.min() == 0 and flips.max() == 10 and len(np.unique(flips)) == 11
    # at every step of every descent the chosen child is at least 8 bits nearer than any sibling: no tie and no near tie decides a
    # descent here (ties are tie_fan's business), so a wrong answer on this tree is a wrong walk, not a coin toss
    cs, ch = vocab["child_start"], vocab["children"]
    leaves = np.flatnonzero(vocab["word_id"] >= 0)
    for i in range(len(desc)):
        p = bt.path(vocab, leaves[want[i]])
        for parent, chosen in zip(p[:-1], p[1:]):
            kids = ch[cs[parent]:cs[parent + 1]]
            dist = np.unpackbits(vocab["desc"][kids] ^ desc[i][None], axis=1).sum(1)
            rest = dist[kids != chosen]
            assert len(rest) == 0 or dist[kids == chosen][0] + 8 <= rest.min()


def test_ragged_covers_every_side_of_the_node_level(oracle, ragged):
    """for each levelsup the leaf lies above, on and below level depth - levelsup wherever the tree has such a leaf, and the node id is the
    root, the leaf itself, and the ancestor at that level respectively"""
    vocab, desc, want = ragged
    level, _ = bt.levels(vocab)
    leaves = np.flatnonzero(vocab["word_id"] >= 0)
    leaf_level = level[leaves[want]]
    assert sorted(np.unique(leaf_level).tolist()) == [1, 2, 3]
    seen = {}
    for levelsup in LEVELSUP:
        nid_level = vocab["depth"] - levelsup
        w, _, nd = oracle.bow_transform(vocab, desc, levelsup)
        assert np.array_equal(w, want)
        above, on, below = leaf_level < nid_level, leaf_level == nid_level, leaf_level > nid_level
        seen[levelsup] = (bool(above.any()), bool(on.any()), bool(below.any()))
        assert (nd[above] == 0).all() and np.array_equal(nd[on], leaves[want[on]])
        if nid_level <= 0:
            assert (nd == 0).all()
        else:
            for i in np.flatnonzero(below):
                assert nd[i] == bt.path(vocab, leaves[want[i]])[nid_level]
    # leaves at levels 1, 2, 3 against node levels 4, 3, 2, 1, 0, -1: every combination the tree allows
    assert seen == {0: (True, False, False), 1: (True, True, False), 2: (True, True, True), 3: (False, True, True), 4: (False, False, True),
                    5: (False, False, True)}


def test_ragged_wavefronts_mix_path_lengths_and_chunk_counts(ragged):
    vocab, desc, want = ragged
    leaves = np.flatnonzero(vocab["word_id"] >= 0)
    chunks = [bt.chunk_counts(vocab, leaves[w]) for w in want]
    assert {c for cc in chunks for c in cc} == {1, 2, 3}
    mixed, three_wide = [], 0
    for g in range(0, len(desc), bt.ROWS):
        grp = chunks[g:g + bt.ROWS]
        lengths = {len(c) for c in grp}
        assert lengths == {1, 2, 3}                               # every group: leaves at levels 1, 2 and 3
        per_level = [{c[l] for c in grp if len(c) > l} for l in range(3)]
        if max(len(s) for s in per_level) >= 2:
            mixed.append(g // bt.ROWS)
            three_wide += 3 in per_level[2]
    # 80 of the 128 level-3 leaves hang under 2-chunk nodes, so not every pair of them can differ; at least half the groups do, several of
    # them with the 3-chunk node, and the first two groups (inside every prefix of 8 and more) are among them
    assert len(mixed) >= len(desc) // bt.ROWS // 2 and three_wide >= 8 and mixed[:2] == [0, 1]
    assert max(bt.RAGGED_PREFIXES) <= len(desc) and min(bt.RAGGED_PREFIXES) == 1


@pytest.mark.parametrize("n", bt.TIE_FAN_SIZES)
def test_tie_fan_oracle_keeps_the_first_of_equals(oracle, n):
    vocab, desc, want = bt.tie_fan(n)
    sets = bt.tie_fan_sets(n)
    assert len(sets) == len(desc) and sets[:n] == [(i,) for i in range(n)] and sets[-1] == tuple(range(n))
    assert set(sets) >= {(i, j) for i in range(n) for j in range(i + 1, n)}
    if n > 37:
        assert {(5, 21), (5, 37), (21, 37), (15, 16), (31, 32), (5, 21, 37)} <= set(sets)
    kid_bits = np.unpackbits(vocab["desc"][1:], axis=1)
    assert (kid_bits.sum(1) == 5).all() and (kid_bits.sum(0) <= 1).all()
    dist = (np.unpackbits(desc, axis=1)[:, None, :] != kid_bits[None]).sum(2)
    for q, s in enumerate(sets):
        inside = np.zeros(n, bool)
        inside[list(s)] = True
        assert (dist[q, inside] == 5 * len(s) - 5).all() and (dist[q, ~inside] == 5 * len(s) + 5).all()
    for levelsup in (0, 1):
        w, wt, nd = oracle.bow_transform(vocab, desc, levelsup)
        assert np.array_equal(w, want) and np.array_equal(wt, vocab["weight"][1 + want])
        assert np.array_equal(nd, (1 + want) if levelsup == 0 else np.zeros_like(want))


@pytest.mark.parametrize("n", bt.FAR_SIZES)
def test_far_oracle_takes_the_first_child(oracle, n):
    vocab, desc, want = bt.far(n)
    assert (np.unpackbits(vocab["desc"][1:][None] ^ desc[:, None], axis=2).sum(2) == 256).all()
    w, wt, nd = oracle.bow_transform(vocab, desc, 0)
    assert (want == 0).all() and np.array_equal(w, want) and (nd == 1).all() and (wt == vocab["weight"][1]).all()


@pytest.mark.parametrize("n", bt.WIDE_SIZES)
def test_wide_oracle_returns_the_stated_winners(oracle, n):
    vocab, desc, want = bt.wide(n)
    assert np.diff(vocab["child_start"])[0] == n
    asked = list(dict.fromkeys([0, 15, 16, 255, 256, n - 2, n - 1]))
    stated = [255 if i == 256 else 17 if (i == n - 1 and n - 1 != 256) else i for i in asked]
    assert want.tolist() == stated and np.array_equal(desc, vocab["desc"][1:][asked])
    assert np.array_equal(vocab["desc"][1 + 256], vocab["desc"][1 + 255])
    assert len(np.unique(vocab["desc"][1:], axis=0)) == n - (1 if n - 1 == 256 else 2)
    w, wt, nd = oracle.bow_transform(vocab, desc, 0)
    assert np.array_equal(w, want) and np.array_equal(nd, 1 + want) and np.array_equal(wt, vocab["weight"][1 + want])


def _all_cases():
    return [("ragged", bt.ragged)] + bt.flat_cases()


@pytest.mark.parametrize("name,build", _all_cases(), ids=[c[0] for c in _all_cases()])
def test_second_restatement_equals_the_oracle_on_the_edge_trees(oracle, name, build):
    """Fails on `ragged` with a restatement that copies the current node of EVERY feature when the level counter reaches depth - levelsup:
    a feature that stopped at a shallower leaf keeps the root (rule 29)."""
    vocab, desc, _ = build()
    for levelsup in LEVELSUP + (2**31 - 1,):
        w, wt, nd = oracle.bow_transform(vocab, desc, levelsup)
        gw, gwt, gnd = nv.bow_transform(vocab, desc, levelsup)
        assert np.array_equal(gw, w) and np.array_equal(gwt, wt) and np.array_equal(gnd, nd), (name, levelsup)


# ---- ovs_vocab_create: the child list must be a tree (checked on the host; status only, no handle is kept) -----------------------------------------
def _create_status(child_start, children, n_nodes, depth=3):
    from openvslam_amd import _lib
    L = _lib.lib()
    cs, ch = np.asarray(child_start, np.int32), np.asarray(children, np.int32)
    desc, weight, word = np.zeros((n_nodes, 32), np.uint8), np.ones(n_nodes), np.full(n_nodes, -1, np.int32)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = L.ovs_vocab_create(0, n_nodes, p(cs), p(ch), p(desc), p(weight), p(word), depth, 16, C.byref(h))
    if st == 0:
        L.ovs_vocab_destroy(h)
    else:
        assert not h.value
    return st


INVALID = -1


def test_vocab_create_refuses_a_cycle():
    """0 -> 1 -> 2 -> 1 ...: every entry is a valid non-root id, the counts fit, and a descent would never end"""
    assert _create_status([0, 1, 2, 3], [1, 2, 1], 3) == INVALID


def test_vocab_create_refuses_a_node_listed_twice():
    assert _create_status([0, 2, 2, 2], [1, 1], 3) == INVALID              # twice under one parent
    assert _create_status([0, 2, 3, 3, 3], [1, 2, 2], 4) == INVALID        # under two parents (a DAG, not a tree)
    assert _create_status([0, 1, 2, 2], [0, 2], 3) == INVALID              # the root as a child: the check that was there before


def test_vocab_create_accepts_the_same_arrays_as_a_tree():
    """past validation: no device here, a handle on a GPU machine"""
    assert _create_status([0, 1, 2, 2], [1, 2], 3) in (0, -2)               # the chain 0 -> 1 -> 2
    assert _create_status([0, 2, 2, 2], [1, 2], 3) in (0, -2)
    assert _create_status([0, 2, 3, 3, 3], [1, 2, 3], 4) in (0, -2)
