"""The sequential pose-graph optimiser reference (tests/posegraph_ref.py; DESIGN.md 3.19, rules G1 to G11) checked on its own, and what the
device shares with it held to it without a device: ovs_det_log against libm and against its exact rationals, the Sim3 logarithm against the
exponential, the first Levenberg-Marquardt step against a dense numpy solve, a stand-alone host program built from
openvslam_amd/csrc/pose_graph_math.inc that must give the reference's bits, the planted poses on the consistent rings, the paths the scene
set reaches, io.pose_graph_problem on a hand-made map, the host plan under the sanitizers, and the argument errors and the C++ class's
degraded result, which need no device."""
import ctypes as C
import math
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import posegraph_ref as ref
import posegraph_scenes as sc
from transform_ref import exp_apply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvslam_amd", "csrc")
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
HOST_SCENES = ["ring12", "dup", "pcg_cap", "noisy24"]
NAN, INF = float("nan"), float("inf")
IDENTITY = ref.state([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], 1.0)


def _sides(x):
    return [math.nextafter(x, 0.0), x, math.nextafter(x, INF)]


# both sides of every step of G4's range reduction: the powers of two, RN(sqrt 2) 2^k, the subnormal border; the NaN cases; a grid
LOG_GRID = ([x for k in (-1074, -1023, -1022, -1021, -54, -2, -1, 0, 1, 2, 54, 1023) for x in _sides(2.0 ** k) if x > 0.0] +
            [x for k in (-1022, -3, -2, -1, 0, 1, 2, 500) for x in _sides(ref.SQRT2 * 2.0 ** k)] +
            [5e-324, 1.7976931348623157e308, 0.0, -0.0, -1.0, -5e-324, INF, -INF, NAN, 1.0, 0.25, 4.0, math.e, 1e-5, 1.00001, 0.99999] +
            [0.25 + 3.75 * k / 256.0 for k in range(257)])

# G3's four branches and both sides of d = 1 - eps (theta = acos(1 - 1e-5) = 4.4721e-3), as exp(u) of the identity; then states that are
# no exponentials: a scale of 1 exactly, a rotation by nearly pi, a NaN
LOG_U = [[1e-7, 2e-7, -1e-7, 0.1, 0.2, 0.3, 1e-13], [1e-7, 2e-7, -1e-7, 0.1, 0.2, 0.3, 0.02], [0.1, 0.2, -0.1, 0.1, 0.2, 0.3, 1e-13],
         [0.1, 0.2, -0.1, 0.1, 0.2, 0.3, 0.02], [4.4e-3, 0.0, 0.0, 0.5, -0.2, 0.1, 0.3], [4.5e-3, 0.0, 0.0, 0.5, -0.2, 0.1, 0.3],
         [0.0, 3.1, 0.0, 1.0, 2.0, 3.0, -0.7], [2.0, -1.0, 0.5, 1.0, 2.0, 3.0, -0.7], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]
LOG_BRANCHES = ["small_theta_small_sigma", "small_theta_large_sigma", "large_theta_small_sigma", "large_theta_large_sigma",
                "small_theta_large_sigma", "large_theta_large_sigma", "large_theta_large_sigma", "large_theta_large_sigma", "small_theta_small_sigma"]


def log_states():
    states = [exp_apply(u, False, IDENTITY) for u in LOG_U]
    states.append(dict(IDENTITY, t=[1.0, 2.0, 3.0]))
    states.append(dict(IDENTITY, R=[NAN, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]))
    states.append(dict(IDENTITY, s=-1.0))
    return states


def ulps(a, b):
    key = lambda x: (lambda u: u if u < 1 << 63 else (1 << 63) - u)(ref.bits(x))
    return abs(key(a) - key(b))


def same_bits(got, want):
    return all((g != g) if w != w else ref.bits(g) == ref.bits(w) for g, w in zip(got, want)) and len(got) == len(want)


# ---- 2: G4
def test_det_log_stays_within_two_ulp_of_libm_on_the_scale_range():
    rng = random.Random(5)
    worst = max(ulps(ref.det_log(x), math.log(x)) for x in (rng.uniform(0.25, 4.0) for _ in range(400000)))
    print("det_log max distance from libm on [0.25, 4]:", worst, "ulp")   # measured: 1
    assert worst <= 2


def test_det_log_coefficients_are_the_exact_rationals_and_the_header_literals():
    text = open(os.path.join(ROOT, "include", "ovs_detmath.h")).read()
    body = text[text.index("OVS_DM_FN double ovs_det_log"):]
    for j in range(1, 11):
        c = float(Fraction(2, 2 * j + 1))
        assert ref.L_K[j] == c and abs(Fraction(c) - Fraction(2, 2 * j + 1)) <= Fraction(math.ulp(c)) / 2   # rounded once, to nearest
        assert c.hex() in body, (j, c.hex())
    assert ref.LN2_HI.hex() in body and ref.LN2_LO.hex() in body and ref.SQRT2.hex() in body
    assert abs(Fraction(ref.LN2_HI) + Fraction(ref.LN2_LO) - Fraction(math.log(2.0))) < Fraction(1, 2 ** 53)   # together ln 2 to more than a double
    assert ref.bits(ref.LN2_HI) & 0x1fffff == 0 and ref.SQRT2 == math.sqrt(2.0)     # 32 significant bits: k ln2_hi is exact for |k| < 2^21


def test_det_log_edges_follow_the_rule():
    for x in (0.0, -0.0, -1.0, -5e-324, INF, -INF, NAN):
        assert ref.det_log(x) != ref.det_log(x), x
    assert ref.det_log(1.0) == 0.0
    for x in LOG_GRID:
        if x > 0.0 and x < INF:
            assert abs(ref.det_log(x) - math.log(x)) <= 4e-16 * max(1.0, abs(math.log(x))), x   # every reduction step lands on the function
    assert ref.det_log(5e-324) == math.log(5e-324) and ulps(ref.det_log(1.7976931348623157e308), math.log(1.7976931348623157e308)) <= 1


# ---- 1: the shared algebra through a plain host compiler
def host_input(grid, states, names):
    flat = [float(len(grid))] + list(grid) + [float(len(states))]
    for S in states:
        flat += list(S["R"]) + list(S["t"]) + [S["s"]]
    flat.append(float(len(names)))
    for n in names:
        s = sc.scene(n)
        flat += [len(s["V"]), len(s["edges"]), len(s["lm_ref"]), s["fix_scale"], s["num_iter"], s["pcg_max_iter"]]
        for key in ("V", "nc"):
            for R, t, c in s[key]:
                flat += list(R) + list(t) + [c]
        flat += s["fixed"]
        for i, j in s["edges"]:
            flat += [i, j]
        for R, t, c in s["meas"]:
            flat += list(R) + list(t) + [c]
        flat += s["lm_ref"]
        for p in s["lm_pos"]:
            flat += list(p)
    return np.array(flat, np.float64)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """(det_log values, logarithms, results) of the host program, built here from the shared file by the plain host compiler."""
    tmp = tmp_path_factory.mktemp("posegraph_host")
    exe = str(tmp / "posegraph_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "posegraph_host.cc")])
    states = log_states()
    host_input(LOG_GRID, states, HOST_SCENES).tofile(str(tmp / "in.bin"))
    subprocess.check_call([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], timeout=300)
    out = np.fromfile(str(tmp / "out.bin"), np.float64).tolist()
    n0, n1 = len(LOG_GRID), len(LOG_GRID) + 7 * len(states)
    results, at = [], n1
    for n in HOST_SCENES:
        s = sc.scene(n)
        size = 13 * len(s["V"]) + 3 * len(s["lm_ref"]) + 8
        results.append(out[at:at + size])
        at += size
    assert at == len(out)
    return out[:n0], [out[n0 + 7 * k:n0 + 7 * k + 7] for k in range(len(states))], results


def test_host_program_gives_det_logs_bits(host):
    assert same_bits(host[0], [ref.det_log(x) for x in LOG_GRID])


def test_host_program_gives_the_logarithms_bits(host):
    states = log_states()
    seen = []
    for S, got in zip(states, host[1]):
        e, branch = ref.log_parts(S)
        seen.append(branch)
        assert same_bits(got, e), (S, got, e)
    assert seen[:len(LOG_BRANCHES)] == LOG_BRANCHES and set(seen) == set(LOG_BRANCHES)
    d = lambda S: 0.5 * (((S["R"][0] + S["R"][4]) + S["R"][8]) - 1.0)
    assert d(states[4]) > 1.0 - ref.EPS > d(states[5])                  # both sides of the small-angle switch
    assert all(x != x for x in host[1][-1][3:]) and all(x != x for x in host[1][-2][:6])   # the log of a negative scale is a NaN; a NaN runs through


@pytest.mark.parametrize("k", range(len(HOST_SCENES)))
def test_host_program_gives_a_whole_optimisations_bits(host, k):
    want = sc.solved(HOST_SCENES[k])[1]
    assert want["info"][0] >= 1
    got = ["nan" if x != x else ref.bits(x) for x in host[2][k]]
    assert got == sc.result_bits(want)


# ---- 3: N-version
def test_logarithm_inverts_the_exponential_on_every_branch():
    """log(exp(u)) = u. The small-angle branch stops at the first order in theta (omega = dR / 2), so its theta is 2.4e-7 as in 3.11's check.
    Measured worst case of the reference over these cases: 4.2e-14 absolute, on the rotation by 3.1, where d is near -1 and both acos(d) and
    sqrt(1 - d d) lose digits (the other cases stay below 9e-16); asserted at 100 times that."""
    worst, seen = 0.0, set()
    for u in LOG_U[:4] + LOG_U[6:]:
        e, branch = ref.log_parts(exp_apply(u, False, IDENTITY))
        seen.add(branch)
        worst = max(worst, max(abs(a - b) for a, b in zip(e, u)))
    print("log(exp(u)) - u, worst:", worst)
    assert seen == set(LOG_BRANCHES) and worst <= 100 * 4.2e-14


@pytest.fixture(scope="module")
def first_ring12():
    opt, _ = sc.solved("ring12")
    return opt, opt.first


def dense_system(opt, lin, lam):
    free = opt.free
    at = {v: 7 * k for k, v in enumerate(free)}
    H, g = np.zeros((7 * len(free), 7 * len(free))), np.zeros(7 * len(free))
    for v in free:
        H[at[v]:at[v] + 7, at[v]:at[v] + 7] = np.array(lin["H"][v]) + lam * np.eye(7)
        g[at[v]:at[v] + 7] = lin["g"][v]
    for ei, A in lin["A"].items():
        i, j = opt.q["edges"][ei]
        H[at[i]:at[i] + 7, at[j]:at[j] + 7] += np.array(A)
        H[at[j]:at[j] + 7, at[i]:at[i] + 7] += np.array(A).T
    return H, g, at


def test_first_step_equals_a_dense_solve(first_ring12):
    """The PCG's step of ring12's first iteration against numpy.linalg.solve on the dense system assembled from the reference's blocks. The PCG
    stops at a preconditioned residual of 1e-6 relative (measured here: 9.3e-7), and the preconditioned system's condition number is 637, so
    the steps may differ by up to their product: the reference shows a relative difference of 5.5e-5 in the largest component (the numpy
    model of the issue, on its own rings, showed 1e-7 to 4e-6); asserted at 100 times the measured figure."""
    opt, lin = first_ring12
    H, g, at = dense_system(opt, lin, lin["lambda"])
    x = np.linalg.solve(H, g)
    mine = np.concatenate([lin["x"][v] for v in opt.free])
    rel = float(np.abs(mine - x).max() / np.abs(x).max())
    print("first step, relative difference from the dense solve:", rel)
    r = g - H @ mine
    assert float(np.linalg.norm(r) / np.linalg.norm(g)) <= 1e-5            # the residual the stopping rule leaves (measured: 9.1e-7)
    assert rel <= 100 * 5.5e-5
    assert np.array_equal(H, H.T)                       # the assembled H is symmetric, bit for bit
    assert np.all(np.linalg.eigvalsh(H) > 0)


def test_column_six_is_exactly_zero_under_fix_scale():
    opt, res = sc.solved("ring12_fixscale")
    lin = opt.first
    for Ji, Jj in lin["J"]:
        for J in (Ji, Jj):
            if J is not None:
                assert all(ref.bits(J[r][6]) & 0x7fffffffffffffff == 0 for r in range(7))
    assert all(lin["x"][v][6] == 0.0 for v in opt.free)
    assert all(s == 1.0 for _, _, s in res["V"])


# ---- 4: the consistent rings
@pytest.mark.parametrize("name", ["ring5", "ring12", "ring40"])
def test_consistent_ring_returns_the_planted_poses_and_landmarks(name):
    """Measured worst cases of the reference: 1.1e-14 over the poses' entries (ring40) and 1.7e-14 over the landmarks' (ring12); the numpy model
    of the issue reached 4e-15 and 2e-14. Asserted at 100 times the measured figures."""
    opt, res = sc.solved(name)
    s = sc.scene(name)
    err = max(abs(a - b) for (R, t, c), (R2, t2, c2) in zip(res["V"], s["true"]) for a, b in zip(list(R) + list(t) + [c], list(R2) + list(t2) + [c2]))
    lerr = max([abs(a - b) for p, q in zip(res["lm"], s["lm_true"]) for a, b in zip(p, q)] or [0.0])
    print(name, "pose error", err, "landmark error", lerr)
    assert err <= 100 * 1.1e-14 and lerr <= 100 * 1.7e-14
    start = max(abs(a - b) for (R, t, c), (R2, t2, c2) in zip(s["V"], s["true"]) for a, b in zip(list(R) + list(t) + [c], list(R2) + list(t2) + [c2]))
    assert start > 0.05                                 # the start was far from it
    for it, qmax, failed, accepted, chi, chi_new in opt.trial_log:
        assert not accepted or chi_new < chi            # chi falls at every accepted trial
    assert opt.paths & {"ten_rejections", "rho_zero", "iteration_cap"}
    if "iteration_cap" in opt.paths:
        assert res["info"][0] == s["num_iter"]
    else:
        assert opt.trial_log[-1][1] == 9 or "rho_zero" in opt.paths


# ---- 5: what the scene set reaches
@pytest.mark.parametrize("name", sc.NAMES)
def test_every_scene_ends_by_the_rules(name):
    """(Also the one place a scene's reference result is computed: solved() caches it for the tests below and for the device tests.)"""
    opt, res = sc.solved(name)
    it, trials, chi0, chi, lam, pcg_total, pcg_last, status = res["info"]
    assert len(opt.trial_log) == trials and it <= sc.scene(name)["num_iter"] and pcg_last <= pcg_total
    for _, qmax, failed, accepted, before, after in opt.trial_log:
        assert qmax < 10 and (not accepted or after < before)          # chi falls at every accepted trial
    if status == 0.0:
        assert opt.paths & {"ten_rejections", "rho_zero", "iteration_cap"} and (chi <= chi0) and lam > 0.0
    else:
        assert it == 0 and trials == 0


def test_scene_set_reaches_every_path():
    paths = set()
    for name in sc.NAMES:
        opt, res = sc.solved(name)
        paths |= opt.paths
    assert paths >= {"accepted_first_trial", "rejected_first_trial", "rejected_later_trial", "accepted_later_trial", "ten_rejections", "rho_zero",
                     "iteration_cap", "pcg_cap", "pcg_zero_iterations", "nothing_to_do", "non_finite"}, paths
    assert ref.LOG_PATHS == set(LOG_BRANCHES)
    info = lambda n: sc.solved(n)[1]["info"]
    assert info("all_fixed")[7] == info("no_edges")[7] == 1.0 and info("nan_edge")[7] == 2.0 and info("ring5")[7] == 0.0
    assert info("pcg_cap")[6] == 3.0 and info("many_edges")[6] == 20.0
    assert len(sc.scene("ring40")["edges"]) == 115 and len(sc.scene("many_edges")["edges"]) == 1100 and len(sc.scene("hub")["edges"]) == 70
    assert [len(sc.scene(n)["edges"]) for n in ("edges63", "edges64", "edges65")] == [63, 64, 65]
    assert [len(sc.scene(n)["V"]) for n in ("verts64", "verts65")] == [64, 65]
    assert sorted({len(sc.scene(n)["lm_ref"]) for n in sc.NAMES}) == [0, 1, 3, 65]
    s = sc.scene("ring12")
    assert -1 in s["lm_ref"] and 0 in s["lm_ref"] and s["fixed"][0] == 1
    # a result that did nothing or met a NaN is its input
    for n in ("all_fixed", "no_edges", "nan_edge"):
        assert sc.result_bits(dict(sc.solved(n)[1], lm=[], info=[]))[:13 * len(sc.scene(n)["V"])] == \
            sc.result_bits(dict(V=sc.scene(n)["V"], lm=[], info=[]))
    # isolated: the free vertex without an edge keeps its state (a lambda-only pivot, a zero step)
    assert sc.solved("isolated")[1]["V"][5] == sc.scene("isolated")["V"][5] and "pivot_failed" not in sc.solved("isolated")[0].paths


# ---- 6: io.pose_graph_problem on a hand-made map
def _shared(pairs):
    """lm_ids per keyframe realising the given covisibility weights: every pair gets landmarks of its own."""
    ids = {}
    nxt = 1000
    for (a, b), w in pairs.items():
        for k in (a, b):
            ids.setdefault(k, []).extend(range(nxt, nxt + w))
        nxt += w
    return ids


def loop_map():
    """(db, (loop id, current id, non_corrected, pre_corrected, loop_connections)): eight keyframes on the ring, a chain as the spanning tree,
    one earlier loop edge 5 - 2, weights 150 along the chain, 120 two apart, 60 three apart, 110 on the loop edge, 105 between 7 and 1, 40
    between 6 and 0; the loop closes 7 on 0, keyframes 6 and 7 are the corrected neighbourhood."""
    from openvslam_amd import io as oio
    from openvslam_amd.ba import rot_to_quat
    n = 8
    true = [sc.planted(v, n) for v in range(n)]
    drifted = [true[0]] + [exp_apply(sc.drift(v, n, 1.0, with_scale=False), True, true[v]) for v in range(1, n)]
    weights = {}
    for v in range(n):
        for k, w in ((1, 150), (2, 120), (3, 60)):
            if v + k < n:
                weights[(v, v + k)] = w
    weights[(2, 5)] = 110
    weights[(1, 7)] = 105
    weights[(0, 6)] = 40
    shared = _shared(weights)
    db = oio.map_database()
    for v in range(n):
        R = np.array(drifted[v]["R"]).reshape(3, 3)
        db.keyframes[v] = oio.keyframe(id=v, rot_cw=rot_to_quat(R), trans_cw=np.array(drifted[v]["t"]), lm_ids=np.array(shared.get(v, []), np.int64),
                                       span_parent=v - 1, span_children=[v + 1] if v + 1 < n else [], loop_edges={2: [5], 5: [2]}.get(v, []))
    lm_ref, pts = sc.landmarks(n, 12)
    for m, (r, p) in enumerate(zip(lm_ref, pts)):
        db.landmarks[m] = oio.landmark(id=m, first_keyfrm=max(r, 0), pos_w=np.array(p), ref_keyfrm=r if r >= 0 else 99)
    as_arg = lambda S: (np.array(S["R"]).reshape(3, 3), np.array(S["t"]), S["s"])
    pose_of = lambda v: (oio.quat_to_rot(db.keyframes[v].rot_cw), db.keyframes[v].trans_cw, 1.0)
    non_corrected = {6: pose_of(6), 7: pose_of(7)}
    pre_corrected = {6: as_arg(true[6]), 7: as_arg(true[7])}
    return db, (0, 7, non_corrected, pre_corrected, {7: [1, 0], 6: [0]})


def scene_of_problem(q, num_iter, fix_scale=0, pcg_max_iter=0):
    states = lambda r, t, s: [(r[i].tolist(), t[i].tolist(), float(s[i])) for i in range(len(s))]
    return dict(V=states(q["rot"], q["trans"], q["scale"]), nc=states(q["nc_rot"], q["nc_trans"], q["nc_scale"]), fixed=q["fixed"].tolist(),
                edges=[tuple(e) for e in q["edge_ij"].tolist()], meas=states(q["edge_rot"], q["edge_trans"], q["edge_scale"]), fix_scale=fix_scale,
                num_iter=num_iter, pcg_max_iter=pcg_max_iter, lm_ref=q["lm_ref"].tolist(), lm_pos=q["lm_pos"].tolist())


def test_pose_graph_problem_builds_upstreams_graph():
    from openvslam_amd import io as oio
    db, args = loop_map()
    q = oio.pose_graph_problem(db, *args)
    # written out by hand from the map above: (a) 6 - 0 has weight 40 and is dropped, 7 - 0 is the current / loop pair, 7 - 1 has 105;
    # then per keyframe its parent, its earlier loop edge, its covisibilities two apart (120); 5 - 2 (110) is a loop edge and no covisibility,
    # 7 - 1 (105) was inserted by (a), everything three apart has 60
    assert [tuple(e) for e in q["edge_ij"].tolist()] == [(7, 0), (7, 1), (1, 0), (2, 1), (2, 0), (3, 2), (3, 1), (4, 3), (4, 2), (5, 4), (5, 2), (5, 3),
                                                         (6, 5), (6, 4), (7, 6), (7, 5)]
    assert q["edge_class"] == ["loop", "loop", "parent", "parent", "covis", "parent", "covis", "parent", "covis", "parent", "loop_edge", "covis",
                               "parent", "covis", "parent", "covis"]
    assert q["keyfrm_ids"] == list(range(8)) and q["fixed"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert q["lm_ids"] == list(range(12)) and q["lm_ref"].tolist() == [0, 1, 2, -1, 4, 5, 6, 7, 0, 1, -1, 3]
    assert q["scale"].tolist() == [1.0] * 8
    non_corrected, pre_corrected = args[2], args[3]
    for k in (6, 7):   # the corrected neighbourhood starts from pre_corrected
        assert np.array_equal(q["rot"][k].reshape(3, 3), pre_corrected[k][0]) and np.array_equal(q["trans"][k], pre_corrected[k][1])
    assert np.allclose(q["rot"][3].reshape(3, 3), oio.quat_to_rot(db.keyframes[3].rot_cw), atol=0, rtol=0)
    sim3 = lambda R, t, s: ([float(v) for v in np.ravel(R)], [float(v) for v in t], float(s))
    start = [sim3(q["rot"][k], q["trans"][k], q["scale"][k]) for k in range(8)]
    m = lambda e: sim3(q["edge_rot"][e], q["edge_trans"][e], q["edge_scale"][e])
    prod, inv = oio._sim3_product, oio._sim3_inverse
    assert m(0) == prod(start[0], inv(start[7]))                                   # a loop connection: the start states
    assert m(14) == prod(sim3(*non_corrected[6]), inv(sim3(*non_corrected[7])))    # 7's parent: both non-corrected
    assert m(12) == prod(start[5], inv(sim3(*non_corrected[6])))                   # 6's parent: 6 non-corrected, 5 has only its pose
    assert m(10) == prod(start[2], inv(start[5]))                                  # the earlier loop edge
    # the reference spreads this loop's correction: the drifted chain and the closing edges disagree, so chi falls to a minimum that is not zero
    want = ref.optimize(scene_of_problem(q, num_iter=6))
    assert want["info"][7] == 0.0 and want["info"][0] >= 1 and want["info"][3] < want["info"][2]


# ---- 7: the host plan under the sanitizers
def test_plan_host_runs_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program with its own main on this CPU, AddressSanitizer and UndefinedBehaviorSanitizer linked in; the test puts nothing
    into the child's environment. It holds the incidence CSR to a brute-force count, every argument error and the arena's order."""
    exe = str(tmp_path / "posegraph_plan_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "posegraph_plan_host.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok" and r.stderr == "", r.stdout + r.stderr
    for name in ("dup", "hub", "ring40"):   # the scenes' lists against the reference's
        opt = sc.solved(name)[0]
        e = np.array(sc.scene(name)["edges"], np.int32)
        np.concatenate([np.array([opt.n_v, opt.n_e], np.int32), e.ravel()]).tofile(str(tmp_path / "graph.bin"))
        r = subprocess.run([exe, str(tmp_path / "graph.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        rows, inc = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
        assert [inc[rows[v]:rows[v + 1]] for v in range(opt.n_v)] == [[2 * ei + side for ei, side in opt.inc[v]] for v in range(opt.n_v)]


# ---- 8: without a device
def test_argument_errors_come_before_the_device():
    from openvslam_amd import _lib
    L = _lib.lib()
    a = sc.arrays(sc.scene("dup"))
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    outs = [np.full(27, -7.0), np.full(9, -7.0), np.full(3, -7.0), np.full(9, -7.0), np.full(8, -7.0)]

    def call(handle=None, num_iter=3, **kw):
        g = dict(a)
        g.update(kw)
        return L.ovs_posegraph_optimize(handle, 3, vp(g["rot"]), vp(g["trans"]), vp(g["scale"]), vp(g["fixed"]), vp(g["nc_rot"]), vp(g["nc_trans"]),
                                        vp(g["nc_scale"]), 4, vp(g["edge_ij"]), vp(g["edge_rot"]), vp(g["edge_trans"]), vp(g["edge_scale"]), 0, num_iter, 0,
                                        3, vp(g["lm_ref"]), vp(g["lm_pos"]), vp(outs[0]), vp(outs[1]), vp(outs[2]), vp(outs[3]), vp(outs[4]))

    assert call() == -1                                      # no handle
    P = C.c_void_p()
    assert L.ovs_posegraph_create(0, 0, 4, 3, C.byref(P)) == -1 and L.ovs_posegraph_create(0, 3, -1, 3, C.byref(P)) == -1
    assert L.ovs_posegraph_create(0, 3, 4, 3, None) == -1 and L.ovs_posegraph_create(-1, 3, 4, 3, C.byref(P)) == -2
    assert L.ovs_posegraph_destroy(None) == -1
    assert all((o == -7.0).all() for o in outs)


def test_cpp_class_without_its_device_leaves_the_map_untouched(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CPP, "test_posegraph_shim"])
    got, _ = run_shim(os.path.join(CPP, "test_posegraph_shim"), tmp_path, device=99)
    db, args = loop_map()
    assert got["failed_calls"] >= 1 and got["normal_updates"] == [0.0] * 12
    from openvslam_amd import io as oio
    for v in range(8):
        R = oio.quat_to_rot(db.keyframes[v].rot_cw)
        assert got["poses"][v][:3, :3].tolist() == R.tolist() and got["poses"][v][:3, 3].tolist() == db.keyframes[v].trans_cw.tolist()
    assert [p.tolist() for p in got["lm"]] == [db.landmarks[m].pos_w.tolist() for m in range(12)]


def run_shim(exe, tmp_path, device=None, num_iter=6):
    """The C++ class on loop_map(): (what it left in the map, the bit patterns the reference expects of a device run)."""
    from openvslam_amd import io as oio
    db, (loop_id, curr_id, non_corrected, pre_corrected, loop_connections) = loop_map()
    flat = [0.0, float(num_iter), float(loop_id), float(curr_id), float(len(db.keyframes))]
    for v in sorted(db.keyframes):
        kf = db.keyframes[v]
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = oio.quat_to_rot(kf.rot_cw), kf.trans_cw
        w = db.covisibility_weights(v)
        flat += [float(v)] + pose.ravel().tolist() + [float(kf.span_parent), float(len(kf.span_children))] + [float(c) for c in kf.span_children]
        flat += [float(len(kf.loop_edges))] + [float(c) for c in kf.loop_edges] + [float(len(w))] + [float(x) for k in sorted(w) for x in (k, w[k])]
    for sims in (non_corrected, pre_corrected):
        flat.append(float(len(sims)))
        for k in sorted(sims):
            R, t, s = sims[k]
            flat += [float(k)] + np.ravel(R).tolist() + np.ravel(t).tolist() + [float(s)]
    flat.append(float(len(loop_connections)))
    for k, conn in loop_connections.items():
        flat += [float(k), float(len(conn))] + [float(c) for c in conn]
    flat.append(float(len(db.landmarks)))
    for m in sorted(db.landmarks):
        lm = db.landmarks[m]
        flat += [float(m), float(lm.ref_keyfrm if lm.ref_keyfrm in db.keyframes else -1)] + lm.pos_w.tolist()
    np.array(flat, np.float64).tofile(str(tmp_path / "map.bin"))
    r = subprocess.run([exe, str(tmp_path / "map.bin"), str(tmp_path / "out.bin")] + ([str(device)] if device is not None else []), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(str(tmp_path / "out.bin"), np.float64)
    n_kf, n_lm = len(db.keyframes), len(db.landmarks)
    poses = [out[16 * v:16 * v + 16].reshape(4, 4) for v in range(n_kf)]
    lm = out[16 * n_kf:16 * n_kf + 4 * n_lm].reshape(n_lm, 4)
    got = dict(poses=poses, lm=[row[:3] for row in lm], normal_updates=lm[:, 3].tolist(), failed_calls=int(out[-1]))
    got["bits"] = [ref.bits(float(x)) for P in poses for x in P[:3].ravel()] + [ref.bits(float(x)) for row in lm for x in row[:3]]
    q = oio.pose_graph_problem(db, loop_id, curr_id, non_corrected, pre_corrected, loop_connections)
    res = ref.optimize(scene_of_problem(q, num_iter=num_iter))
    want = []
    for R, t, s in res["V"]:
        for r_ in range(3):
            want += [ref.bits(x) for x in R[3 * r_:3 * r_ + 3]] + [ref.bits(t[r_] / s)]
    want += [ref.bits(x) for p in res["lm"] for x in p]
    return got, want
