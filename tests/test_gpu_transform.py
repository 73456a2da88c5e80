"""The Sim3 transform optimiser on the device (csrc/sim3_opt.hip, openvslam_amd.solve, cpp/openvslam/optimize/transform_optimizer.h) against
the sequential reference tests/transform_ref.py: the inlier count and the flags for equality, R12, t12, s12 and the eight doubles of out_info as
uint64 bit patterns. Every scene is one of tests/transform_scene_io.py's CASES, whose distance from the gate and from the Huber switch is
asserted in tests/test_transform_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_ref
import transform_ref as tr
import transform_scene_io as io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
INVALID, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def solve():
    from openvslam_amd import solve
    return solve


def device_problem(solve, prob):
    cam = lambda c: solve.camera(**c)
    arr = lambda key, w: np.array(prob[key], np.float64).reshape(-1, w)
    return dict(p1=arr("p1", 3), p2=arr("p2", 3), obs1=arr("obs1", 2), obs2=arr("obs2", 2), w1=np.array(prob["w1"], np.float32),
                w2=np.array(prob["w2"], np.float32), cam_1=cam(prob["cam_1"]), cam_2=cam(prob["cam_2"]), R=prob["R"], t=prob["t"], s=prob["s"])


def of_device(r):
    bits = lambda v: sim3_ref.bits(float(v))
    return dict(num_inliers=int(r["num_inliers"]), R=[bits(v) for v in np.ravel(r["rot_12"])], t=[bits(v) for v in r["trans_12"]], s=bits(r["scale_12"]),
                info=[bits(v) for v in r["info"]], flags=[int(f) for f in r["outlier_flags"]])


def same(got, want):
    """Equality of two result_bits dicts; a NaN in out_info is a NaN whatever its payload."""
    nan = lambda u: (u & 0x7ff0000000000000) == 0x7ff0000000000000 and (u & 0xfffffffffffff) != 0
    info = all(a == b or (nan(a) and nan(b)) for a, b in zip(got["info"], want["info"]))
    return info and {k: v for k, v in got.items() if k != "info"} == {k: v for k, v in want.items() if k != "info"}


def run(solve, name, handle=None):
    return solve.optimize_transform_batch([device_problem(solve, io.problem(name))], io.CASES[name][1], io.CHI_SQ, io.NUM_ITER, handle=handle)[0]


def expected(name):
    return io.result_bits(io.solved(name)[1])


# ---- the lanes' edges (a third round of lanes at 129), both values of fix_scale, both camera models, every path of rules 7 and 8
@pytest.mark.parametrize("name", ["n0", "n9", "n10", "n12", "n63", "n64", "n65", "n129", "n65_fixed", "equirect", "mixed", "clean", "too_few",
                                  "r1_rejected"])
def test_result_equals_the_reference_bit_for_bit(solve, name):
    got, want = of_device(run(solve, name)), expected(name)
    assert same(got, want), (got, want)
    if name in ("n0", "n9", "too_few"):
        q = io.problem(name)
        assert got["num_inliers"] == 0 and got["R"] == [sim3_ref.bits(v) for v in q["R"]] and got["s"] == sim3_ref.bits(q["s"])   # the input, untouched
    else:
        assert got["num_inliers"] >= 10 and got["info"][4] != 0


# ---- a batch against its problems one by one
def test_batch_equals_its_problems_solved_alone(solve):
    probs = [device_problem(solve, io.problem(name)) for name in io.BATCH]
    assert [len(q["w1"]) for q in probs] == [65, 0, 9, 12, 64]
    got = solve.optimize_transform_batch(probs, False, io.CHI_SQ, io.NUM_ITER)
    for name, q, g in zip(io.BATCH, probs, got):
        alone = solve.optimize_transform_batch([q], False, io.CHI_SQ, io.NUM_ITER)[0]
        assert of_device(g) == of_device(alone)
        assert same(of_device(g), expected(name))


# ---- a NaN ends nothing
def test_nan_point_is_flagged_and_the_call_returns(solve):
    got, want = of_device(run(solve, "nan_point")), expected("nan_point")
    assert same(got, want) and got["flags"][17] == 1
    assert all(np.isfinite(v) for v in run(solve, "nan_point")["rot_12"].ravel())


# ---- one handle, many calls
def test_same_handle_same_bytes(solve):
    h = solve._transform_handle(2, 160)
    a, b, c = of_device(run(solve, "n65", handle=h)), of_device(run(solve, "n129", handle=h)), of_device(run(solve, "n65", handle=h))
    assert a == c and same(a, expected("n65")) and same(b, expected("n129"))
    r = solve.optimize_transform_batch([device_problem(solve, io.problem("n12"))], False, io.CHI_SQ, io.NUM_ITER, handle=h, with_info=False)[0]
    assert r["info"] is None and r["num_inliers"] == io.solved("n12")[1]["num_inliers"]


# ---- capacity and argument errors leave the handle usable
def test_error_contract(solve):
    from openvslam_amd import _lib
    L = _lib.lib()
    h = solve._transform_handle(2, 70)
    ok = lambda: same(of_device(run(solve, "n65", handle=h)), expected("n65"))
    assert ok()
    q = device_problem(solve, io.problem("n65"))
    n = 65
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cams = (_lib.Camera * 3)(q["cam_1"], q["cam_1"], q["cam_1"])
    rot, trans, scale = np.tile(np.eye(3), (3, 1, 1)), np.zeros((3, 3)), np.ones(3)
    out_i, out_d = np.full(4, -7, np.int32), [np.full(36, -7.0) for _ in range(4)]
    flags = np.full(256, 9, np.uint8)

    def call(P=1, offsets=(0, n), p1=q["p1"], obs1=q["obs1"], w1=q["w1"], cams_1=cams, rot_in=rot, chi_sq=10.0, iters=10, num=out_i, flags=flags,
             info=out_d[3], handle=h._h):
        opt = lambda a: None if a is None else vp(a)
        off = None if offsets is None else np.array(offsets, np.int32)
        return L.ovs_sim3opt_optimize_batch(handle, P, opt(off), opt(p1), vp(q["p2"]), opt(obs1), vp(q["obs2"]), opt(w1), vp(q["w2"]), cams_1, cams,
                                            opt(rot_in), vp(trans), vp(scale), 0, chi_sq, iters, opt(num), vp(out_d[0]), vp(out_d[1]), vp(out_d[2]),
                                            opt(flags), opt(info))

    assert call(handle=None) == INVALID
    for kw in (dict(offsets=None), dict(p1=None), dict(obs1=None), dict(w1=None), dict(cams_1=None), dict(rot_in=None), dict(num=None), dict(flags=None)):
        assert call(**kw) == INVALID, kw
    assert call(P=-1) == INVALID
    assert call(offsets=(1, n)) == INVALID and call(P=2, offsets=(0, 40, 30)) == INVALID
    assert call(iters=0) == INVALID and call(chi_sq=0.0) == INVALID and call(chi_sq=float("nan")) == INVALID and call(chi_sq=float("inf")) == INVALID
    bad_model = (_lib.Camera * 1)(solve.camera(2, 458, 457, 367, 248))
    nan_fx = (_lib.Camera * 1)(solve.camera(0, float("nan"), 457, 367, 248))
    no_rows = (_lib.Camera * 1)(solve.camera(1, cols=1920, rows=0))
    for bad in (bad_model, nan_fx, no_rows):
        assert call(cams_1=bad) == INVALID
    assert call(P=3, offsets=(0, 20, 40, 60)) == CAPACITY           # more problems than the handle was created for
    assert call(offsets=(0, 71)) == CAPACITY                        # more matches (refused before anything is read)
    assert (out_i == -7).all() and all((a == -7.0).all() for a in out_d) and (flags == 9).all()   # nothing truncated, nothing written
    assert call(P=0) == 0 and (out_i == -7).all()                   # no problems: nothing to do
    assert call(P=2, offsets=(0, 0, 0), info=None) == 0             # no matches is not an error; out_info may be NULL
    assert out_i[:2].tolist() == [0, 0] and (out_d[3] == -7.0).all()
    assert ok()
    with pytest.raises(_lib.OvsError):
        solve.optimize_transform_batch([q, q, q], False, handle=h)


# ---- the Python class and the constructor's helper
def test_python_class(solve):
    q = device_problem(solve, io.problem("n64"))
    num, R, t, s, flags = solve.transform_optimizer(False, io.NUM_ITER).optimize(q, io.CHI_SQ)
    want = io.solved("n64")[1]
    assert num == want["num_inliers"] and flags.astype(int).tolist() == want["flags"]
    assert [sim3_ref.bits(float(v)) for v in list(R.ravel()) + list(t) + [s]] == [sim3_ref.bits(v) for v in want["R"] + want["t"] + [want["s"]]]
    prob, idx1 = io.problem_of(io.keyframe_pair("kf20"))
    assert len(idx1) == 20 and same(of_device(run(solve, "kf20")), expected("kf20"))


# ---- the C++ class
def test_cpp_class_returns_the_reference_results(tmp_path):
    cpp = os.path.join(ROOT, "openvslam_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp] + (["asan"] if SUFFIX else ["test_transform_shim"]))
    names = ["kf20", "kf64"]
    pairs = [io.keyframe_pair(k) for k in names]
    io.write_scene(tmp_path / "scene.bin", pairs, False, io.NUM_ITER, io.CHI_SQ)
    r = subprocess.run([os.path.join(cpp, "test_transform_shim" + SUFFIX), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ABI calls failed 0" in r.stdout, r.stdout + r.stderr
    got = io.read_results(tmp_path / "out.bin", len(names))
    for p, (k, pair) in enumerate(zip(names, pairs)):
        want, idx1 = io.solved(k)[1], io.problem_of(pair)[1]
        kept = [1 if j >= 0 else 0 for j in pair["matched"]]
        for i, f in zip(idx1, want["flags"]):
            kept[i] = 0 if f else 1            # an outlier's landmark is nulled; the match to the erased landmark was never collected and stays
        for run_ in ("single", "batch"):
            g = got[run_][p]
            assert g["num_inliers"] == want["num_inliers"] >= 10 and g["kept"] == kept
            assert g["R"] + g["t"] + [g["s"]] == [sim3_ref.bits(v) for v in want["R"] + want["t"] + [want["s"]]]


# ---- ids 6 to 8 of the device self-test
def test_det_functions_on_the_device_equal_the_restatement():
    from openvslam_amd import _lib
    from test_transform_ref import DET_GRID, FNS
    L = _lib.lib()
    for fn in (6, 7, 8):
        xs = np.array([x for f, x in DET_GRID if f == fn] + list(np.linspace(-0.8, 0.8, 4001)) + list(np.linspace(-40.0, 40.0, 2001)))
        out = np.zeros_like(xs)
        assert L.ovs_detmath_eval(0, fn, xs.ctypes.data_as(C.c_void_p), None, out.ctypes.data_as(C.c_void_p), len(xs)) == 0
        for x, y in zip(xs.tolist(), out.tolist()):
            want = FNS[fn](x)
            assert (y != y) if want != want else sim3_ref.bits(y) == sim3_ref.bits(want), (fn, x)
