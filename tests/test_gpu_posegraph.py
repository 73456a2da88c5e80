"""The pose-graph optimiser on the device (csrc/pose_graph.hip, openvslam_amd.pose_graph, cpp/openvslam/optimize/graph_optimizer.h) against the
sequential reference tests/posegraph_ref.py: the optimised (R, t, s) of every vertex, the corrected landmarks and the eight doubles of out_info
as uint64 bit patterns, on every scene of tests/posegraph_scenes.py (whose coverage of the rules' paths tests/test_posegraph_ref.py asserts)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import posegraph_ref as ref
import posegraph_scenes as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
INVALID, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def pgm():
    from openvslam_amd import pose_graph
    return pose_graph


def run(opt, name):
    a = sc.arrays(sc.scene(name))
    return opt.optimize_arrays(a["rot"], a["trans"], a["scale"], a["fixed"], a["nc_rot"], a["nc_trans"], a["nc_scale"], a["edge_ij"], a["edge_rot"],
                               a["edge_trans"], a["edge_scale"], a["lm_ref"], a["lm_pos"], a["num_iter"], a["pcg_max_iter"], a["fix_scale"])


def of_device(r):
    R, t, s, lm, info = r
    flat = [x for v in range(len(s)) for x in R[v].ravel().tolist() + t[v].tolist() + [float(s[v])]] + lm.ravel().tolist() + info.tolist()
    return ["nan" if x != x else ref.bits(x) for x in flat]


def expected(name):
    return sc.result_bits(sc.solved(name)[1])


def input_bits(name):
    s = sc.scene(name)
    return ["nan" if x != x else ref.bits(x) for R, t, sc_ in s["V"] for x in list(R) + list(t) + [sc_]]


@pytest.fixture(scope="module")
def big(pgm):
    return pgm.graph_optimizer(False, max_vertices=320, max_edges=1200, max_landmarks=128)


# ---- 1: every scene, every output
@pytest.mark.parametrize("name", sc.NAMES)
def test_result_equals_the_reference_bit_for_bit(big, name):
    got, want = of_device(run(big, name)), expected(name)
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:8]


# ---- 2 to 4: one handle, many calls; capacity does not show; nothing stale
def test_same_handle_twice_gives_the_same_bytes(big):
    assert of_device(run(big, "ring12")) == of_device(run(big, "ring12")) == expected("ring12")


def test_large_and_exactly_sized_handles_agree(pgm, big):
    s = sc.scene("dup")
    exact = pgm.graph_optimizer(False, max_vertices=len(s["V"]), max_edges=len(s["edges"]), max_landmarks=len(s["lm_ref"]))
    assert exact._cap == (3, 4, 3)
    assert of_device(run(exact, "dup")) == of_device(run(big, "dup")) == expected("dup")
    assert exact._cap == (3, 4, 3)


def test_a_scene_after_a_larger_one_gives_its_own_bytes(pgm):
    h = pgm.graph_optimizer(False, max_vertices=80, max_edges=128, max_landmarks=70)
    assert of_device(run(h, "hub")) == expected("hub")
    assert of_device(run(h, "ring5")) == expected("ring5")
    assert of_device(run(h, "ring12")) == expected("ring12")
    assert of_device(run(h, "pair")) == expected("pair")


# ---- 5: a NaN ends nothing
def test_nan_edge_returns_the_input_with_status_two(big):
    R, t, s, lm, info = run(big, "nan_edge")
    assert info[7] == 2.0 and info[0] == 0.0 and info[1] == 0.0 and info[2] != info[2]
    assert of_device((R, t, s, lm, info))[:13 * len(s)] == input_bits("nan_edge")


# ---- 6: the error contract through the ABI
def test_error_contract(pgm):
    from openvslam_amd import _lib
    L = _lib.lib()
    h = pgm.graph_optimizer(False, max_vertices=5, max_edges=10, max_landmarks=3)
    ok = lambda: of_device(run(h, "ring5")) == expected("ring5")
    assert ok() and h._cap == (5, 10, 3)
    a = sc.arrays(sc.scene("two_fixed"))   # 5 vertices, 10 edges, 3 landmarks
    outs = [np.full(45, -7.0), np.full(15, -7.0), np.full(5, -7.0), np.full(9, -7.0), np.full(8, -7.0)]
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)

    def call(handle=h._h, n_v=5, n_e=10, n_l=3, num_iter=3, pcg=0, **kw):
        g = dict(a, out_rot=outs[0], out_trans=outs[1], out_scale=outs[2], out_lm=outs[3], info=outs[4])
        g.update(kw)
        return L.ovs_posegraph_optimize(handle, n_v, vp(g["rot"]), vp(g["trans"]), vp(g["scale"]), vp(g["fixed"]), vp(g["nc_rot"]), vp(g["nc_trans"]),
                                        vp(g["nc_scale"]), n_e, vp(g["edge_ij"]), vp(g["edge_rot"]), vp(g["edge_trans"]), vp(g["edge_scale"]), 0, num_iter,
                                        pcg, n_l, vp(g["lm_ref"]), vp(g["lm_pos"]), vp(g["out_rot"]), vp(g["out_trans"]), vp(g["out_scale"]),
                                        vp(g["out_lm"]), vp(g["info"]))

    untouched = lambda: all((o == -7.0).all() for o in outs)
    assert call(handle=None) == INVALID
    for key in ("rot", "trans", "scale", "fixed", "nc_rot", "nc_trans", "nc_scale", "edge_ij", "edge_rot", "edge_trans", "edge_scale", "lm_ref", "lm_pos",
                "out_rot", "out_trans", "out_scale", "out_lm"):
        assert call(**{key: None}) == INVALID, key
    assert call(n_v=-1) == INVALID and call(n_e=-1) == INVALID and call(n_l=-1) == INVALID
    assert call(num_iter=0) == INVALID and call(pcg=-1) == INVALID
    ij = a["edge_ij"].copy()
    ij[3, 1] = 5
    assert call(edge_ij=ij) == INVALID                       # an index out of range
    ij[3, 1] = -1
    assert call(edge_ij=ij) == INVALID
    ij[3] = (2, 2)
    assert call(edge_ij=ij) == INVALID                       # i == j
    assert call(n_v=4) == INVALID                            # the edges now point beyond the vertices
    for bad in (5, -2):
        lm_ref = a["lm_ref"].copy()
        lm_ref[1] = bad
        assert call(lm_ref=lm_ref) == INVALID
    fixed = a["fixed"].copy()
    fixed[4] = 2
    assert call(fixed=fixed) == INVALID
    assert untouched()
    big5 = {k: (np.concatenate([v, v]) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    assert call(n_v=6, n_e=0, n_l=0, **{k: big5[k] for k in ("rot", "trans", "scale", "fixed", "nc_rot", "nc_trans", "nc_scale")}) == CAPACITY
    assert call(n_e=11, **{k: big5[k] for k in ("edge_ij", "edge_rot", "edge_trans", "edge_scale")}) == CAPACITY
    assert call(n_l=4, **{k: big5[k] for k in ("lm_ref", "lm_pos")}) == CAPACITY
    assert untouched()                                       # nothing truncated, nothing written
    assert call(info=None) == 0                              # out_info may be NULL
    assert (outs[4] == -7.0).all() and not (outs[0] == -7.0).any()
    assert call(n_v=0, n_e=0, n_l=0, rot=None, edge_ij=None, lm_ref=None) == 0 and outs[4][7] == 1.0   # nothing at all: nothing to do
    assert ok()
    P = C.c_void_p()
    assert L.ovs_posegraph_create(0, 0, 1, 1, C.byref(P)) == INVALID and L.ovs_posegraph_create(0, 1, -1, 0, C.byref(P)) == INVALID
    assert L.ovs_posegraph_create(0, 1, 1, 1, None) == INVALID and L.ovs_posegraph_destroy(None) == INVALID


# ---- 7: the Python class over io.pose_graph_problem, and the C++ class
def test_python_class_over_a_map_database(pgm):
    import test_posegraph_ref as tp
    from openvslam_amd import io as oio
    db, args = tp.loop_map()
    q = oio.pose_graph_problem(db, *args)
    poses, lms, info = pgm.graph_optimizer(False).optimize(q, num_iter=6)
    want = ref.optimize(tp.scene_of_problem(q, num_iter=6))
    assert info.tolist()[:2] == want["info"][:2] and [ref.bits(x) for x in info.tolist()] == [ref.bits(x) for x in want["info"]]
    for i, k in enumerate(q["keyfrm_ids"]):
        R, t, s = want["V"][i]
        assert [ref.bits(x) for x in poses[k][0].ravel().tolist() + poses[k][1].tolist()] == [ref.bits(x) for x in list(R) + [t[0] / s, t[1] / s, t[2] / s]]
    for i, l in enumerate(q["lm_ids"]):
        assert [ref.bits(x) for x in lms[l].tolist()] == [ref.bits(x) for x in want["lm"][i]]
    assert info[0] >= 1 and info[3] < info[2]


def test_cpp_class_returns_the_reference_results(tmp_path):
    import test_posegraph_ref as tp
    cpp = os.path.join(ROOT, "openvslam_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp] + (["asan"] if SUFFIX else ["test_posegraph_shim"]))
    got, want = tp.run_shim(os.path.join(cpp, "test_posegraph_shim" + SUFFIX), tmp_path)
    assert got["failed_calls"] == 0 and got["bits"] == want


# ---- 8: id 9 of the device self-test
def test_det_log_on_the_device_equals_the_restatement():
    from openvslam_amd import _lib
    from test_posegraph_ref import LOG_GRID
    L = _lib.lib()
    xs = np.array(LOG_GRID + list(np.linspace(0.25, 4.0, 4001)) + list(np.geomspace(1e-300, 1e300, 2001)))
    out = np.zeros_like(xs)
    assert L.ovs_detmath_eval(0, 9, xs.ctypes.data_as(C.c_void_p), None, out.ctypes.data_as(C.c_void_p), len(xs)) == 0
    for x, y in zip(xs.tolist(), out.tolist()):
        want = ref.det_log(x)
        assert (y != y) if want != want else ref.bits(y) == ref.bits(want), x
