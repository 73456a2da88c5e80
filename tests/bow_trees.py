"""Hand-built vocabularies and queries for the BoW transform's edges (tests/test_bow_trees.py on the CPU, tests/test_gpu_bow_edges.py on the
device): plain numpy, fixed seeds. Every builder returns (vocab, desc, want_word): a vocabulary in synth.synth_vocabulary's dict layout
(child_start, children, desc, weight, word_id, depth; node ids in creation order, children of a node consecutive, word ids in leaf order, so
tools/vocab_io.py can write it), the query descriptors, and the word each query was built to reach, so that a test can hold those facts
against the oracle without running the code under test.

What synth.synth_vocabulary never has: a leaf above the last level, a declared depth beyond the deepest leaf, inner nodes of 1, 15..17 and
31..33 children side by side (the kernel gives one 16-lane row to a descriptor and walks a node's children in chunks of 16), ties made on
purpose, a child position beyond 255."""
import itertools

import numpy as np

CHUNK = 16      # children per pass of the kernel's chunk loop (one lane each)
ROWS = 4        # descriptors per 64-lane wavefront (one 16-lane row each)

TIE_FAN_SIZES = (2, 16, 17, 32, 33, 48)
FAR_SIZES = (2, 17)
WIDE_SIZES = (257, 4097)
RAGGED_PREFIXES = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65)


def _flip(rng, desc, k):
    """a copy of a 32-byte descriptor with exactly k distinct bits flipped"""
    bits = np.unpackbits(desc)
    bits[rng.permutation(256)[:k]] ^= 1
    return np.packbits(bits)


def _pack(kids, desc, weight, depth):
    n = len(kids)
    child_start = np.zeros(n + 1, np.int32)
    children = []
    for i in range(n):
        children.extend(kids[i])
        child_start[i + 1] = len(children)
    leaves = [i for i in range(n) if not kids[i]]
    word_id = -np.ones(n, np.int32)
    word_id[leaves] = np.arange(len(leaves), dtype=np.int32)
    w = np.zeros(n)
    w[leaves] = np.asarray(weight, np.float64)[leaves]
    return dict(child_start=child_start, children=np.asarray(children, np.int32), desc=np.stack(desc).astype(np.uint8), weight=w,
                word_id=word_id, depth=int(depth))


def _flat(n, child_desc, depth=1):
    """root + n leaves with the given descriptors; distinct weights that are exact in float32 (the binary formats store floats)"""
    kids = [list(range(1, n + 1))] + [[] for _ in range(n)]
    desc = [np.zeros(32, np.uint8)] + list(child_desc)
    return _pack(kids, desc, 1.0 + 0.25 * np.arange(n + 1), depth)


def levels(vocab):
    """level of every node (root 0) and its parent (-1 for the root)"""
    cs, ch = vocab["child_start"], vocab["children"]
    n = len(vocab["word_id"])
    level, parent = np.zeros(n, np.int64), -np.ones(n, np.int64)
    for p in range(n):                      # parents come before their children
        c = ch[cs[p]:cs[p + 1]]
        level[c], parent[c] = level[p] + 1, p
    return level, parent


def depth_on_disk(vocab, fmt):
    """the depth a reader reports for `vocab` written as `fmt`: DBoW2's text and binary headers carry L; an FBoW file has no such field and
    the reader reports the level of the deepest node"""
    return int(levels(vocab)[0].max()) if fmt == "fbow" else int(vocab["depth"])


def path(vocab, node):
    """root ... node"""
    _, parent = levels(vocab)
    out = [int(node)]
    while parent[out[-1]] >= 0:
        out.append(int(parent[out[-1]]))
    return out[::-1]


def chunk_counts(vocab, node):
    """passes of the 16-wide chunk loop at every step of the descent to `node`"""
    cs = vocab["child_start"]
    return [-(-int(cs[p + 1] - cs[p]) // CHUNK) for p in path(vocab, node)[:-1]]


RAGGED_FANS = (15, 32, 33, 31)     # leaves under C's four inner children: 1, 2, 3 and 2 chunks


def ragged(seed=7):
    """Declared depth 4, deepest leaf at level 3. root -> A (a leaf at level 1), B (one child B1 with 17 leaves), C (16 children: a leaf,
    four inner nodes with 15, 32, 33 and 31 leaves, eleven more leaves). A child's descriptor is its parent's with 40 bits flipped; every
    thirteenth word has weight 0. 256 queries in 64 aligned groups of four (the four rows of one wavefront): A's descriptor, a level-2 leaf of
    C, and two level-3 leaves taken in turn from B1 and C's inner children, each with 0 to 10 bits flipped."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kids, desc = [[]], [rng.integers(0, 256, 32, dtype=np.uint8)]

    def add(parent):
        desc.append(_flip(rng, desc[parent], 40))
        kids.append([])
        kids[parent].append(len(desc) - 1)
        return len(desc) - 1

    a, b, c = add(0), add(0), add(0)                        # level 1
    b1 = add(b)                                             # level 2
    c_kids = [add(c) for _ in range(16)]
    inner = c_kids[1:5]
    fans = [[add(b1) for _ in range(17)]]                   # level 3
    for node, k in zip(inner, RAGGED_FANS):
        fans.append([add(node) for _ in range(k)])
    n = len(desc)
    weight = 0.5 + 0.125 * rng.integers(0, 64, n)           # exact in float32
    vocab = _pack(kids, desc, weight, 4)
    vocab["weight"][np.flatnonzero(vocab["word_id"] % 13 == 5)] = 0.0
    shallow = [c_kids[0]] + c_kids[5:]
    deep = [x for group in itertools.zip_longest(*fans) for x in group if x is not None]     # B1, C15, C32, C33, C31 in turn
    assert len(deep) % 2 == 0
    src = []
    for g in range(len(deep) // 2):
        src += [a, shallow[g % len(shallow)], deep[2 * g], deep[2 * g + 1]]
    q = np.stack([_flip(rng, vocab["desc"][s], i % 11) for i, s in enumerate(src)])
    return vocab, q, vocab["word_id"][src].copy()


def _union(n, members):
    bits = np.zeros(256, np.uint8)
    for i in members:
        bits[5 * i:5 * i + 5] = 1
    return np.packbits(bits)


def tie_fan_sets(n):
    """the member sets S of tie_fan(n)'s queries, in query order"""
    sets = [(i,) for i in range(n)] + list(itertools.combinations(range(n), 2))
    triples = [(0, 1, 2), (1, 8, 15), (15, 16, 17), (5, 21, 37), (15, 31, 47), (16, 32, 47), (14, 30, 46), (n - 3, n - 2, n - 1)]
    sets += [t for t in dict.fromkeys(triples) if 0 <= t[0] and t[2] < n]
    sets.append(tuple(range(n)))
    return sets


def tie_fan(n):
    """Depth 1, n <= 51 children; child i has exactly bits [5i, 5i + 5) set. A query that is the union of the blocks of a set S is at distance
    5|S| - 5 from every child in S and 5|S| + 5 from every other child: the children in S tie at the minimum and word min(S) wins. Queries:
    every single, every pair, a few triples (same lane of different chunks, chunk boundaries), all children."""
    assert 2 <= n and 5 * n <= 256
    vocab = _flat(n, [_union(n, (i,)) for i in range(n)])
    sets = tie_fan_sets(n)
    return vocab, np.stack([_union(n, s) for s in sets]), np.array([min(s) for s in sets], np.int32)


def far(n, seed=3):
    """Depth 1; every child is the complement of the query: every distance is 256 (the largest key the reduction sees) and child 0 wins."""
    rng = np.random.Generator(np.random.PCG64(seed))
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    vocab = _flat(n, [~q] * n)
    return vocab, np.stack([q] * 5), np.zeros(5, np.int32)


def wide(n, seed=11):
    """Depth 1, one node with n > 256 children of distinct random descriptors, except that child 256 repeats child 255 (the earlier one wins
    across the 8-bit position boundary) and, where the last child is not child 256 itself, the last child repeats child 17. Queries: exact
    copies of children 0, 15, 16, 255, 256, n - 2 and n - 1."""
    assert n > 256
    rng = np.random.Generator(np.random.PCG64(seed))
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    assert len(np.unique(d, axis=0)) == n
    d[256] = d[255]
    winner = {256: 255}
    if n - 1 != 256:
        d[n - 1] = d[17]
        winner[n - 1] = 17
    vocab = _flat(n, list(d))
    asked = list(dict.fromkeys([0, 15, 16, 255, 256, n - 2, n - 1]))
    return vocab, d[asked].copy(), np.array([winner.get(i, i) for i in asked], np.int32)


def flat_cases():
    """[(name, builder)] of every depth-1 tree"""
    return ([("tie_fan_%d" % n, lambda n=n: tie_fan(n)) for n in TIE_FAN_SIZES] + [("far_%d" % n, lambda n=n: far(n)) for n in FAR_SIZES]
            + [("wide_%d" % n, lambda n=n: wide(n)) for n in WIDE_SIZES])
