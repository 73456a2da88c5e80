"""The sequential reference of the monocular initialiser's pose recovery (tests/reconstruct_ref.py; DESIGN.md 3.15, rules R1 to R12) checked on
its own, and the algebra the device shares (openvslam_amd/csrc/reconstruct_math.inc) held to it without a device: every scene a device test
uses keeps every gate a relative 1e-9 away from its threshold, so that no last-bit difference could flip a flag, a count or the winner; the
Jacobi route agrees with numpy's SVD on the hypotheses and the winner, which is the planted motion; a stand-alone host program built from the
shared file by the plain host compiler gives the reference's bits on every case. Plus the C ABI's argument errors, which are decided before
the device is touched."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import reconstruct_io as io
import reconstruct_ref as ref
import reconstruct_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
MARGIN_MIN, OFF_MAX = 1e-9, 1e-13
NOISY_THR = (2.0, 4.0)
MIN_ABOVE = ("f65", 66)     # min_num_triangulated one above the winner's count


def every_use():
    """Every (case, parameters) under which a device test solves a scene."""
    uses = [(name, {}) for name in sc.CASES]
    uses += [(name, dict(reproj_err_thr=thr)) for name in ("h_noisy", "f_noisy") for thr in NOISY_THR]
    uses.append((MIN_ABOVE[0], dict(min_num_triangulated=MIN_ABOVE[1])))
    return uses


# ---- what makes the bit comparison sound
@pytest.mark.parametrize("name,params", every_use(), ids=lambda v: v if isinstance(v, str) else "-".join("%s" % x for x in v.values()) or "default")
def test_every_use_keeps_its_distance_from_every_decision(name, params):
    r, margin, stats, info = sc.solved(name, **params)
    assert stats.get("off", 0.0) <= OFF_MAX
    for gate, value in margin.items():   # cos, depth, reproj, ratio, similar, parallax
        assert value >= MARGIN_MIN, (gate, value)
    assert info.get("distinct", True)
    print(name, params, {k: "%.3g" % v for k, v in margin.items()}, "off %.3g" % stats.get("off", 0.0))


def test_smallest_margins_over_all_uses():
    """The figures DESIGN.md 3.15 quotes."""
    worst, off = {}, 0.0
    for name, params in every_use():
        _, margin, stats, _ = sc.solved(name, **params)
        off = max(off, stats.get("off", 0.0))
        for gate, value in margin.items():
            worst[gate] = min(worst.get(gate, math.inf), value)
    print("smallest relative margins:", {k: "%.3g" % v for k, v in sorted(worst.items())}, "largest off-diagonal residue: %.3g" % off)
    assert set(worst) == {"cos", "depth", "reproj", "ratio", "similar", "parallax"} and min(worst.values()) >= MARGIN_MIN and off <= OFF_MAX


# ---- the scenes reach what their names say
def test_sizes_triangulate_what_they_plant():
    for n in sc.COUNTS:
        h, f = sc.expected("h%d" % n), sc.expected("f%d" % n)
        assert max(h["counts"]) == n and max(f["counts"]) == n
        assert sum(sc.problem("f%d" % n)["inlier"]) == n < len(sc.problem("f%d" % n)["inlier"])      # non-inlier matches in every scene
        assert f["success"] == (1 if n >= 50 else 0) and (f["best"] == 2 or n < 50)
        assert f["counts"][4:] == [0, 0, 0, 0]
    assert sc.expected("h_success")["success"] == 1 and sc.expected("h_success")["best"] == 0
    assert sum(sc.expected("f200")["flags"]) == 200 and sum(sc.expected("h_success")["flags"]) > 30


def test_every_failing_exit_has_its_scene():
    r = sc.expected("h_rotation")
    assert r["counts"] == [0] * 8 and ref.hypotheses(sc.problem("h_rotation")) == [] and r == ref.failed(81)
    r = sc.expected("h_two_similar")
    assert r["success"] == 0 and max(r["counts"]) >= 50 and sum(1 for c in r["counts"] if 0.8 * max(r["counts"]) < c) >= 2
    assert r["counts"].count(max(r["counts"])) == 2      # and a tie at the top: the first of the two would be the winner
    r = sc.expected("f_low_parallax")
    best = r["counts"].index(max(r["counts"]))
    assert r["success"] == 0 and max(r["counts"]) >= 50 and sum(1 for c in r["counts"] if 0.8 * max(r["counts"]) < c) == 1 and 0.0 < r["parallax"][best] < 1.0
    r, above = sc.expected(MIN_ABOVE[0]), sc.expected(MIN_ABOVE[0], min_num_triangulated=MIN_ABOVE[1])
    assert r["success"] == 1 and max(r["counts"]) == MIN_ABOVE[1] - 1 and above["success"] == 0 and above["counts"] == r["counts"]
    assert above["pts"] == ref.failed(81)["pts"] and above["R"] == [0.0] * 9
    r, clean = sc.expected("f_nan"), sc.expected("f50")
    assert clean["success"] == 1 and r["success"] == 0 and r["counts"][2] == clean["counts"][2] - 1 == 49
    for name in ("f0", "h0", "empty"):
        assert sc.expected(name) == ref.failed(len(sc.problem(name)["inlier"]))


def test_gross_matches_fail_the_reprojection_gate_and_the_threshold_matters():
    q, r = sc.problem("f_gross"), sc.expected("f_gross")
    assert r["success"] == 1 and max(r["counts"]) == 65
    assert all(r["flags"][i] == 0 and r["pts"][i] == [0.0, 0.0, 0.0] for i, k in enumerate(q["kinds"]) if k != "good")
    for name in ("h_noisy", "f_noisy"):
        tight, loose = sc.expected(name, reproj_err_thr=2.0), sc.expected(name, reproj_err_thr=4.0)
        assert max(tight["counts"]) < max(loose["counts"]) and ref.as_bits(tight) != ref.as_bits(loose)


def test_chained_cases_select_what_they_should():
    assert sc.chained_problem("p65")["model"] == ref.MODEL_H and sc.chained_problem("c129")["model"] == ref.MODEL_F
    assert sc.expected("c129")["success"] == 1


# ---- the arc cosine restated in Python is the header's
def test_python_acos_is_the_headers():
    from oracle import binding as ob
    xs = [k / 997.0 for k in range(-997, 998)] + [1.0 - 2.0 ** -k for k in range(1, 54)] + [2.0 ** -k for k in range(1, 70)] + [float(np.float32(0.99996192306)), 1.5, -1.5]
    want = ob.detmath_eval(2, xs, None)
    for x, w in zip(xs, want):
        got = ref.det_acos(x)
        assert (got != got and w != w) or ref.bits(got) == ref.bits(float(w)), x
    assert abs(ref.det_acos(0.3) - math.acos(0.3)) < 1e-15 and ref.det_acos(float("nan")) != ref.det_acos(float("nan"))


def test_keys_order_floats():
    xs = [-1.0, -0.5, -0.0, 0.0, 1e-30, 0.5, 0.9999, 1.0]
    keys = [ref.key_of(x) for x in xs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and max(keys) < 0xFFFFFFFF


# ---- N-version: numpy's SVD in place of the Jacobi route
def _numpy_hypotheses(q):
    fx, fy, cx, cy = q["cam"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    M = np.array(q["mat"]).reshape(3, 3)
    out = []
    if q["model"] == ref.MODEL_H:
        U, w, Vt = np.linalg.svd(np.linalg.inv(K) @ M @ K)
        s = np.linalg.det(U) * np.linalg.det(Vt)
        d1, d2, d3 = w
        if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
            return out
        aux1, aux3 = math.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), math.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        root = math.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
        for second in (False, True):
            den = (d1 - d3) * d2 if second else (d1 + d3) * d2
            cs = (d1 * d3 - d2 * d2) / den if second else (d2 * d2 + d1 * d3) / den
            for i, sign in enumerate((1, -1, -1, 1)):
                sn = sign * root / den
                Rp = np.array([[cs, 0, sn], [0, -1, 0], [sn, 0, -cs]]) if second else np.array([[cs, 0, -sn], [0, 1, 0], [sn, 0, cs]])
                tp = np.array([x1[i], 0, x3[i] if second else -x3[i]]) * ((d1 + d3) if second else (d1 - d3))
                t = U @ tp
                out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
        return out
    U, w, Vt = np.linalg.svd(K.T @ M @ K)
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    R1, R2 = U @ W @ Vt, U @ W.T @ Vt
    R1, R2 = (R1 if np.linalg.det(R1) > 0 else -R1), (R2 if np.linalg.det(R2) > 0 else -R2)
    return [(R1, t), (R1, -t), (R2, t), (R2, -t)]


@pytest.mark.parametrize("name", ["h_success", "h65", "h_two_similar", "f65", "f129", "f_low_parallax", "c129"])
def test_hypotheses_and_winner_agree_with_numpy_svd(name):
    q = sc.problem(name)
    mine, theirs = ref.hypotheses(q), _numpy_hypotheses(q)
    assert len(mine) == len(theirs) == (8 if q["model"] == ref.MODEL_H else 4)
    for h in mine:
        R, t = np.array(h["R"]).reshape(3, 3), np.array(h["t"])
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12 and abs(np.linalg.norm(t) - 1.0) < 1e-12
        assert np.abs(np.array(h["c"]) + R.T @ t).max() < 1e-15
    # the same set: the SVD's signs may permute the hypotheses, not change them
    near = lambda a, b: np.abs(a[0] - b[0]).max() < 1e-8 and np.abs(a[1] - b[1]).max() < 1e-8
    as_pair = lambda h: (np.array(h["R"]).reshape(3, 3), np.array(h["t"]))
    assert all(any(near(as_pair(h), o) for o in theirs) for h in mine) and all(any(near(as_pair(h), o) for h in mine) for o in theirs)
    # the winner over numpy's hypotheses is the reference's pose
    want = sc.expected(name)
    thr_sq = ref.f32(16.0)
    res = [ref.check_pose(q, ref._hyp([float(v) for v in R.ravel()], [float(v) for v in t]), thr_sq) for R, t in theirs]
    best = ref.most_plausible([r[0] for r in res], [r[1] for r in res], 1.0, 50)
    assert (best >= 0) == bool(want["success"])
    assert sorted(r[0] for r in res) == sorted(want["counts"][:len(res)])
    if best >= 0:
        assert near(theirs[best], (np.array(want["R"]).reshape(3, 3), np.array(want["t"]))) and res[best][3] == want["flags"]


@pytest.mark.parametrize("name", ["h_success", "f65", "f129", "f200"])
def test_winning_pose_is_the_planted_motion_up_to_scale(name):
    """The planted matrix is exact, so the decomposition returns the motion to rounding; the points are the scene's up to the keypoint noise."""
    q, r = sc.problem(name), sc.expected(name)
    R, t = q["truth"]
    assert r["success"] == 1
    nrm = math.sqrt(sum(v * v for v in t))
    assert max(abs(a - b) for a, b in zip(r["R"], R)) < 1e-9 and max(abs(a - b / nrm) for a, b in zip(r["t"], t)) < 1e-9
    depths = [p[2] * nrm for p, f in zip(r["pts"], r["flags"]) if f]
    assert len(depths) > 30 and all(1.0 < z < 60.0 for z in depths)     # the scene's depths, in the scene's unit


# ---- the shared algebra through a plain host compiler
def test_host_program_gives_the_reference_bits_on_every_case(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CPP, "reconstruct_host"])
    for params in ({}, dict(reproj_err_thr=2.0), dict(min_num_triangulated=MIN_ABOVE[1])):
        names = sorted(sc.CASES) if not params else ["h_noisy", "f_noisy", MIN_ABOVE[0]]
        path = tmp_path / "cases.bin"
        path.write_bytes(io.host_input([sc.problem(k) for k in names], **params))
        r = subprocess.run([os.path.join(CPP, "reconstruct_host"), str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = io.host_output(r.stdout, [len(sc.problem(k)["inlier"]) for k in names])
        for k, g in zip(names, got):
            assert g == ref.as_bits(sc.expected(k, **params)), (k, params)


# ---- the C++ class without a device: the failure policy's "wait for the next frame"
def write_shim_scene(path):
    import test_twoview_ref as tv
    io.write_shim_scene(path, [tv.problem(k) for k in sc.CHAINED], (tv.FOCAL, tv.FOCAL, tv.CX, tv.CY), tv.ITERS, tv.SEED)
    return [len(tv.problem(k)["x1"]) for k in sc.CHAINED]


def test_cpp_class_degrades_without_its_device(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CPP, "test_reconstruct_shim"])
    sizes = write_shim_scene(tmp_path / "scene.bin")
    r = subprocess.run([os.path.join(CPP, "test_reconstruct_shim"), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "99"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "caller error thrown 1" in r.stdout, r.stdout + r.stderr
    for g, n in zip(io.read_shim_results(tmp_path / "out.bin", sizes), sizes):
        assert g == dict(initialised=0, R=[0] * 9, t=[0] * 3, pts=[[0, 0, 0]] * (n + 5), flags=[0] * (n + 5))
    assert "0 initialised" in r.stdout and "ABI calls failed %d, degraded %d" % (len(sizes), len(sizes)) in r.stdout


# ---- the C ABI's argument errors, decided before the device is touched
def test_argument_errors_need_no_device():
    from openvslam_amd import _lib
    L = _lib.lib()
    INVALID, NO_DEVICE = -1, -2
    h = C.c_void_p()
    assert L.ovs_reconstruct_create(0, 0, 100, C.byref(h)) == INVALID and L.ovs_reconstruct_create(0, 4, 0, C.byref(h)) == INVALID
    assert L.ovs_reconstruct_create(0, 4, 100, None) == INVALID and L.ovs_reconstruct_create(0, 1 << 20, 8, C.byref(h)) == INVALID
    assert L.ovs_reconstruct_create(99, 4, 100, C.byref(h)) == NO_DEVICE and not h
    assert L.ovs_reconstruct_create(-1, 4, 100, C.byref(h)) == NO_DEVICE and not h
    assert L.ovs_reconstruct_destroy(None) == INVALID
    none = [None] * 9
    assert L.ovs_reconstruct_batch(None, 1, *none, 4.0, 1.0, 50, *([None] * 8)) == INVALID
    fake = C.c_void_p(1)   # never dereferenced: these are refused before the handle is read
    for thr, par in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (4.0, 0.0), (4.0, float("nan")), (4.0, float("inf"))):
        assert L.ovs_reconstruct_batch(fake, 1, *none, thr, par, 50, *([None] * 8)) == INVALID
    assert L.ovs_reconstruct_batch(fake, 1, *none, 4.0, 1.0, 50, *([None] * 8)) == INVALID      # no offsets
    assert L.ovs_reconstruct_batch(fake, -1, *none, 4.0, 1.0, 50, *([None] * 8)) == INVALID
    with pytest.raises(_lib.OvsError):   # the Python mirror raises: no device 99 anywhere
        from openvslam_amd import solve
        solve._reconstruct_handle(4, 16, device=99)
