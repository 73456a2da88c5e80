"""The pose-graph optimiser's scene set: small graphs, each pinning one edge of the rules, as dicts tests/posegraph_ref.py
reads. Deterministic: every number comes from closed forms of the vertex and edge indices, no random state anywhere. A scene plants world
poses S_v = (R_v, t_v, 1), measures M_ji = S_j S_i^-1 from them (consistent unless a row says otherwise), starts the vertices at
exp(drift_v) S_v with a drift that grows along the graph in rotation, translation and scale, and fixes vertex 0 at its planted pose. The
non-corrected poses are the start; landmark m of reference vertex r is planted at p_m in the world and stored where the non-corrected pose
puts it, nc_r^-1 (S_r p_m), so that a recovered graph returns p_m.

solved(name) caches the reference's result; arrays(scene) are the flat arrays of the C ABI."""
import functools
import math

import numpy as np

import posegraph_ref as ref
from transform_ref import exp_apply

NAN = float("nan")


def planted(v, n):
    """A camera on a circle of radius 4 looking roughly inwards, bobbing a little: S_vw with unit scale."""
    a = 2.0 * math.pi * v / n
    u = [0.1 * math.sin(3.0 * a), a, 0.05 * math.cos(2.0 * a), 0.0, 0.0, 0.0, 0.0]
    S = exp_apply(u, True, ref.state([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], 1.0))
    c = [4.0 * math.cos(a), 0.3 * math.sin(2.0 * a), 4.0 * math.sin(a)]
    t = [-((S["R"][3 * i] * c[0] + S["R"][3 * i + 1] * c[1]) + S["R"][3 * i + 2] * c[2]) for i in range(3)]
    return ref.state(S["R"], t, 1.0)


def drift(v, n, amount, with_rotation=True, with_scale=True):
    f = amount * v / max(n - 1, 1)
    rot = [0.02 * f, -0.01 * f, 0.015 * f] if with_rotation else [0.0, 0.0, 0.0]
    return rot + [0.10 * f, -0.05 * f, 0.08 * f, (0.05 * f if with_scale else 0.0)]


def tup(S):
    return (list(S["R"]), list(S["t"]), S["s"])


def ring_edges(n):
    e = [(v, v + k) for v in range(n) for k in (1, 2, 3) if v + k < n]
    return e + [(n - 1, 0)]


def chain_edges(n_v, n_e):
    """A chain with (v, v + 2), (v, v + 3), ... edges behind it until there are n_e."""
    e = [(v, v + 1) for v in range(n_v - 1)]
    k = 2
    while len(e) < n_e:
        e += [(v, v + k) for v in range(n_v - k)][:n_e - len(e)]
        k += 1
    return e


def landmarks(n_v, count):
    """(lm_ref, planted positions): every seventh unreferenced, the rest dealt round the vertices (the fixed vertex 0 among them)."""
    lm_ref = [-1 if m % 7 == 3 else m % n_v for m in range(count)]
    pts = [[1.5 * math.sin(0.7 * m), 0.4 * math.cos(1.3 * m), 1.5 * math.cos(0.9 * m + 0.2)] for m in range(count)]
    return lm_ref, pts


def make(n_v, edges, amount=1.0, fixed=(0,), fix_scale=0, num_iter=10, pcg_max_iter=0, n_lm=3, noise=0.0, with_rotation=True, with_scale=True):
    true = [planted(v, n_v) for v in range(n_v)]
    meas = []
    for ei, (i, j) in enumerate(edges):
        M = ref.compose_inverse(true[j], true[i])
        if noise:
            u = [noise * math.sin(1.0 + 2.3 * ei + 0.9 * k) for k in range(7)]
            M = exp_apply(u, False, ref.state(M["R"], M["t"], M["s"]))
        meas.append(tup(M))
    fixed_flags = [1 if v in fixed else 0 for v in range(n_v)]
    start = [true[v] if fixed_flags[v] else exp_apply(drift(v, n_v, amount, with_rotation, with_scale), fix_scale, true[v]) for v in range(n_v)]
    lm_ref, pts = landmarks(n_v, n_lm)
    lm_pos = []
    for r, p in zip(lm_ref, pts):
        if r < 0:
            lm_pos.append(list(p))
            continue
        S, nc = true[r], start[r]
        c = [S["s"] * ref.dot3(S["R"][3 * i], S["R"][3 * i + 1], S["R"][3 * i + 2], *p) + S["t"][i] for i in range(3)]
        lm_pos.append([nc["s21"] * ref.dot3(nc["R"][i], nc["R"][3 + i], nc["R"][6 + i], *c) + nc["t21"][i] for i in range(3)])
    return dict(V=[tup(S) for S in start], nc=[tup(S) for S in start], fixed=fixed_flags, edges=list(edges), meas=meas, fix_scale=fix_scale,
                num_iter=num_iter, pcg_max_iter=pcg_max_iter, lm_ref=lm_ref, lm_pos=lm_pos, true=[tup(S) for S in true], lm_true=pts)


def _nan_edge():
    s = make(5, ring_edges(5))
    R, t, sc = s["meas"][2]
    s["meas"][2] = (R, [NAN, t[1], t[2]], sc)
    return s


def _isolated():
    s = make(6, ring_edges(5))   # vertex 5 is free and has no edge: its block is lambda I, its step zero
    return s


def _at_rest():
    """Pure integer translations, exact measurements: every error is exactly zero, so the right-hand side is, the PCG stops before its first
    iteration, the step is zero and the round ends on rho == 0."""
    eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    ts = [[0.0, 0.0, 0.0], [1.0, 2.0, -3.0], [-2.0, 4.0, 1.0]]
    V = [(list(eye), list(t), 1.0) for t in ts]
    edges = [(0, 1), (1, 2), (2, 0)]
    meas = [(list(eye), [ts[j][k] - ts[i][k] for k in range(3)], 1.0) for i, j in edges]
    return dict(V=V, nc=V, fixed=[1, 0, 0], edges=edges, meas=meas, fix_scale=0, num_iter=4, pcg_max_iter=0, lm_ref=[1, -1, 2],
                lm_pos=[[1.0, 1.0, 1.0], [2.0, 0.0, 1.0], [0.5, 0.25, 4.0]], true=V, lm_true=[[1.0, 1.0, 1.0], [2.0, 0.0, 1.0], [0.5, 0.25, 4.0]])


BUILDERS = {
    "pair": lambda: make(2, [(0, 1)], n_lm=1, with_rotation=False),            # (a scale and translation drift: small theta, large sigma)
    "ring5": lambda: make(5, ring_edges(5), n_lm=0),
    "ring12": lambda: make(12, ring_edges(12), n_lm=65),
    "ring40": lambda: make(40, ring_edges(40), num_iter=6),
    "ring12_fixscale": lambda: make(12, ring_edges(12), fix_scale=1, with_scale=False),
    # (noisy24 converges in four iterations and ends on ten rejections at its minimum; Gauss-Newton from lambda = 1e-16 rejects nothing
    # before that on any mild start. far5 starts grossly wrong: trials rejected and then accepted, and the iteration cap. pair_far ends on
    # rho == 0.)
    "noisy24": lambda: make(24, ring_edges(24), noise=0.02, num_iter=8),
    "far5": lambda: make(5, ring_edges(5), noise=0.5, amount=300.0, num_iter=8),
    "pair_far": lambda: make(2, [(0, 1)], amount=200.0, num_iter=8, n_lm=0),
    "edges63": lambda: make(40, chain_edges(40, 63), num_iter=3),
    "edges64": lambda: make(40, chain_edges(40, 64), num_iter=3),
    "edges65": lambda: make(40, chain_edges(40, 65), num_iter=3),
    "verts64": lambda: make(64, chain_edges(64, 80), num_iter=2),
    "verts65": lambda: make(65, chain_edges(65, 80), num_iter=2),
    "hub": lambda: make(71, [((0, k) if k % 3 else (k, 0)) for k in range(1, 71)], fixed=(1,), num_iter=2),
    "dup": lambda: make(3, [(0, 1), (1, 2), (2, 1), (0, 2)]),
    "many_edges": lambda: make(300, chain_edges(300, 1100), amount=0.2, num_iter=2, pcg_max_iter=20),
    "two_fixed": lambda: make(5, ring_edges(5), fixed=(0, 2)),
    "all_fixed": lambda: make(5, ring_edges(5), fixed=(0, 1, 2, 3, 4)),
    "no_edges": lambda: make(3, []),
    "isolated": _isolated,
    "pcg_cap": lambda: make(12, ring_edges(12), pcg_max_iter=3),
    "nan_edge": _nan_edge,
    "at_rest": _at_rest,
}
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def solved(name):
    """(optimizer, result) of the reference on the scene, computed once per process and never modified."""
    opt = ref.Optimizer(scene(name))
    return opt, opt.run()


def arrays(s):
    """The C ABI's input arrays of a scene, C-contiguous."""
    def split(states):
        n = len(states)
        return (np.array([x[0] for x in states], np.float64).reshape(n, 9), np.array([x[1] for x in states], np.float64).reshape(n, 3),
                np.array([x[2] for x in states], np.float64).reshape(n))
    rot, trans, scale = split(s["V"])
    nc_rot, nc_trans, nc_scale = split(s["nc"])
    e_rot, e_trans, e_scale = split(s["meas"])
    return dict(rot=rot, trans=trans, scale=scale, fixed=np.array(s["fixed"], np.uint8), nc_rot=nc_rot, nc_trans=nc_trans, nc_scale=nc_scale,
                edge_ij=np.array(s["edges"], np.int32).reshape(len(s["edges"]), 2), edge_rot=e_rot, edge_trans=e_trans, edge_scale=e_scale,
                fix_scale=int(s["fix_scale"]), num_iter=int(s["num_iter"]), pcg_max_iter=int(s["pcg_max_iter"]),
                lm_ref=np.array(s["lm_ref"], np.int32), lm_pos=np.array(s["lm_pos"], np.float64).reshape(len(s["lm_pos"]), 3))


def result_bits(res):
    """A result as one list of 64-bit patterns: per vertex R, t, s; the landmarks; info (a NaN as the word 'nan', whatever its payload)."""
    flat = [x for R, t, s in res["V"] for x in list(R) + list(t) + [s]] + [x for p in res["lm"] for x in p] + list(res["info"])
    return ["nan" if x != x else ref.bits(x) for x in flat]
