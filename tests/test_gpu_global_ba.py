"""Global bundle adjustment on the device: the conjugate-gradient solver bit for bit against the sequential reference
(tests/ba_pcg_ref.py), ovs_global_ba_optimize against local BA's first round, against the oracle and against the CPU restatement
(tests/global_ba_ref.py), the edges of the call, and the class layers on a saved map."""
import threading

import numpy as np
import pytest

import ba_pcg_ref as ref
import global_ba_ref

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return np.array_equal(ref.bits(a), ref.bits(b))


# ---- A1: the solver, bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.SIZES)
def test_pcg_solve_gives_the_references_bits(n):
    """Below and above 64 entries per row (6 .. 66), 64 and 65 blocks (384, 390), both sides of the Cholesky's limit (1020 .. 1032), one full
    workgroup of the lane-per-block kernels and a second one holding one lane (1536, 1542); the chunk the host queues between two looks at
    the done word changes nothing. (The test entry stages NaN into everything the kernels must not read: the padding columns, the padding
    rows, the padding behind the right-hand side.)"""
    from openvslam_amd import ba
    S, g = ref.case(n)
    want_x, want_info = ref.solved(n)
    x, info = ba.pcg_solve(S, g)
    assert info[:2] == want_info[:2] and ref.bits(info[2]) == ref.bits(want_info[2]), (info, want_info)
    assert _same_bits(x, want_x)
    for check_every in (1, 7):
        x2, info2 = ba.pcg_solve(S, g, check_every=check_every)
        assert _same_bits(x2, want_x) and info2 == info


def test_pcg_solve_stops_at_the_cap_and_says_so():
    from openvslam_amd import ba
    S, g = ref.case(66)
    want_x, want_info = ref.solved(66, max_iter=3)
    for check_every in (0, 1, 2):
        x, info = ba.pcg_solve(S, g, max_iter=3, check_every=check_every)
        assert info == want_info and info[0] == 3 and info[1] is True
        assert _same_bits(x, want_x)


@pytest.mark.parametrize("n", ref.BLOCK_SIZES)
def test_pcg_solve_gives_the_references_bits_on_block_dominant_systems(n):
    """513 blocks (three workgroups of the lane-per-block kernels, the last with one lane) and the capacity (1024 blocks, four full
    workgroups, pitch == n, a system of 302 MB: the default chunk and check_every = 7 only). 15 iterations at both sizes."""
    from openvslam_amd import ba
    assert n // 6 <= ba.pcg_max_free() and (n < 6144 or n // 6 == ba.pcg_max_free())
    S, g = ref.block_case(n)
    want_x, want_info = ref.block_solved(n)
    x, info = ba.pcg_solve(S, g)
    assert info[:2] == want_info[:2] and ref.bits(info[2]) == ref.bits(want_info[2]), (info, want_info)
    assert _same_bits(x, want_x)
    for check_every in (1, 7) if n < 6144 else (7,):
        x2, info2 = ba.pcg_solve(S, g, check_every=check_every)
        assert _same_bits(x2, want_x) and info2 == info


@pytest.mark.parametrize("max_iter,iters,capped", [(125, 125, False), (124, 124, True), (126, 125, False)])
def test_pcg_solve_where_convergence_and_the_cap_meet(max_iter, iters, capped):
    """n = 66 converges in 125 iterations: a cap of 125 is not met, one of 124 is, one of 126 changes nothing. With check_every equal to the
    iteration count the deciding pass is the first of a chunk, with one more the last."""
    from openvslam_amd import ba
    S, g = ref.case(66)
    assert ref.solved(66)[1][:2] == (125, False)
    want_x, want_info = ref.solved(66, max_iter=max_iter)
    assert want_info[:2] == (iters, capped)
    if not capped:
        assert _same_bits(want_x, ref.solved(66)[0]) and want_info == ref.solved(66)[1]
    for check_every in (iters, iters + 1):
        x, info = ba.pcg_solve(S, g, max_iter=max_iter, check_every=check_every)
        assert info[:2] == want_info[:2] and ref.bits(info[2]) == ref.bits(want_info[2]), (check_every, info, want_info)
        assert _same_bits(x, want_x)


def test_pcg_solve_stops_at_the_cap_with_a_second_workgroup():
    from openvslam_amd import ba
    S, g = ref.case(1542)
    want_x, want_info = ref.solved(1542, max_iter=3)
    assert want_info[:2] == (3, True) and 0.0165 < want_info[2] < 0.0166
    for check_every in (0, 1, 2):
        x, info = ba.pcg_solve(S, g, max_iter=3, check_every=check_every)
        assert info == want_info
        assert _same_bits(x, want_x)


# ---- A2: the solver's error contract -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bad pivot", "nan off the diagonal blocks", "nan on the diagonal", "indefinite"])
def test_pcg_solve_failures_found_by_a_later_workgroup(name):
    """1542 unknowns, the offending entries in block 256: lane 0 of the second workgroup of k_pcg_init meets the pivot; the indefinite
    system is one k_pcg_update detects, where workgroup 0 alone records it. Status -1, and a good solve on the same thread afterwards."""
    from openvslam_amd import ba
    from openvslam_amd._lib import OvsError
    M, h = ref.failure_cases(1542)[name]
    with pytest.raises(ref.Failed):
        ref.solve(M, h)
    with pytest.raises(OvsError) as e:
        ba.pcg_solve(M, h)
    assert e.value.status == -1
    S, g = ref.case(1542)
    x, info = ba.pcg_solve(S, g)
    assert _same_bits(x, ref.solved(1542)[0]) and info == ref.solved(1542)[1]


@pytest.mark.parametrize("n", [12, 1542])
def test_pcg_solve_right_hand_side_that_is_not_finite(n):
    """A NaN or an Inf in g (first entry of the last block; 1542: entry 1536, the second workgroup's lane): P4's test is false at k = 0, so it
    is no failure but the outcome of g = 0, on the device as in the reference."""
    from openvslam_amd import ba
    S, g = ref.case(n)
    for v in (np.nan, np.inf):
        h = np.array(g)
        h[n - 6] = v
        want_x, want_info = ref.solve(S, h)
        assert want_info == (0, False, 0.0) and not want_x.any()
        x, info = ba.pcg_solve(S, h)
        assert info == (0, False, 0.0) and _same_bits(x, np.zeros(n))


def test_pcg_solve_error_contract():
    from openvslam_amd import ba
    from openvslam_amd._lib import OvsError
    S, g = ref.case(12)
    want_x = ref.solved(12)[0]
    ind = np.eye(12)
    ind[np.arange(6), np.arange(6) + 6] = ind[np.arange(6) + 6, np.arange(6)] = -3.0   # positive definite blocks, p.q = 12 - 36
    bad_block = np.array(S)
    bad_block[7, 7] = -1.0
    nan = np.array(S)
    nan[1, 8] = nan[8, 1] = np.nan
    nan_block = np.array(S)
    nan_block[3, 3] = np.nan
    for M in (ind, bad_block, nan, nan_block):   # a NaN is a reported failure: the number of launches does not depend on the data
        with pytest.raises(OvsError) as e:
            ba.pcg_solve(M, np.ones(12))
        assert e.value.status == -1
        assert _same_bits(ba.pcg_solve(S, g)[0], want_x)   # a good solve on the same thread afterwards
    for n in (5, 7, 0):
        with pytest.raises(OvsError) as e:
            ba.pcg_solve(np.eye(n), np.ones(n))
        assert e.value.status == -1
    for kw in (dict(tol=0.0), dict(tol=float("nan")), dict(max_iter=-1), dict(check_every=-1)):
        with pytest.raises(OvsError) as e:
            ba.pcg_solve(S, g, **kw)
        assert e.value.status == -1
    x, info = ba.pcg_solve(S, np.zeros(12))
    assert not x.any() and info == (0, False, 0.0)


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------
_scenes = {}


def _scene(stereo_frac, n_pose=10, n_pt=1500, obs=500):
    key = (stereo_frac, n_pose, n_pt, obs)
    if key not in _scenes:
        from test_ba import _lba_scene
        d, mono, st, bf, _, _ = _lba_scene(3, n_pose=n_pose, n_pt=n_pt, obs_per_pose=obs, stereo_frac=stereo_frac)
        _scenes[key] = (d, mono, st, bf)
    return _scenes[key]


def _global(d, mono, st, bf, solver, num_iter=10, huber=None, **kw):
    from openvslam_amd import ba
    hm, hs = ba.huber_deltas(1) if huber is None else huber   # (the scenes pass a baseline: a Stereo rig)
    return ba.global_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], st, bf, hm, hs, num_iter, solver, **kw)


# ---- A3: solver 1 is local BA's first round ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stereo_frac", [0.0, 0.3])
def test_cholesky_path_is_local_bas_first_round_bit_for_bit(stereo_frac):
    from openvslam_amd import ba
    d, mono, st, bf = _scene(stereo_frac)
    want = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], st, bf, num_first_iter=10, num_second_iter=0)
    got = _global(d, mono, st, bf, ba.SOLVER_CHOLESKY)
    assert _same_bits(got["poses"], want["poses"]) and _same_bits(got["points"], want["points"])
    assert got["info"][2] == want["info"][4] >= 3 and got["info"][4] == 1 and got["info"][5] == 0
    assert _same_bits(got["info"][:2], want["info"][:2])


# ---- A4: solver 2 against solver 1 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stereo_frac,n_pose,n_pt,obs", [(0.0, 10, 1500, 500), (0.3, 10, 1500, 500), (0.0, 50, 20000, 2000)])
def test_pcg_path_agrees_with_the_cholesky_path(stereo_frac, n_pose, n_pt, obs):
    """The same LM path (iterations and trials identical) and states within the bound test_local_ba_device_and_host_solver_agree uses
    between two solvers."""
    from openvslam_amd import ba
    d, mono, st, bf = _scene(stereo_frac, n_pose, n_pt, obs)
    chol = _global(d, mono, st, bf, ba.SOLVER_CHOLESKY)
    pcg = _global(d, mono, st, bf, ba.SOLVER_PCG)
    print("info", chol["info"], pcg["info"], "poses %.3g points %.3g" % (np.abs(chol["poses"] - pcg["poses"]).max(), np.abs(chol["points"] - pcg["points"]).max()))
    assert np.array_equal(chol["info"][2:4], pcg["info"][2:4]) and pcg["info"][4] == 2 and pcg["info"][5] > 0 and pcg["info"][6] == 0
    assert np.allclose(chol["poses"], pcg["poses"], rtol=1e-9, atol=1e-10)
    assert np.allclose(chol["points"], pcg["points"], rtol=1e-9, atol=1e-10)


# ---- A5: across the switch ---------------------------------------------------------------------------------------------------------------
N_SWITCH = 3   # LM iterations of the two rings: the host path of local BA factors 1026 unknowns on one core per trial


def test_by_size_takes_the_cholesky_at_1020_unknowns():
    from openvslam_amd import ba
    d = global_ba_ref.ring(171, 4000, 100)
    hm, hs = ba.huber_deltas(0)
    got = ba.global_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], None, 0.0, hm, hs, N_SWITCH, ba.SOLVER_BY_SIZE)
    assert got["info"][4] == 1 and got["info"][5] == 0 and got["info"][2] == N_SWITCH
    want = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], None, 0.0, N_SWITCH, 0)
    assert _same_bits(got["poses"], want["poses"]) and _same_bits(got["points"], want["points"])


def test_by_size_takes_the_pcg_at_1026_unknowns(oracle):
    from oracle import lba
    from openvslam_amd import ba
    from openvslam_amd._lib import OvsError
    d = global_ba_ref.ring(172, 4000, 100)
    hm, hs = ba.huber_deltas(0)
    args = (d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], None, 0.0)
    got = ba.global_ba_optimize(*args, hm, hs, N_SWITCH, ba.SOLVER_BY_SIZE)
    assert got["info"][4] == 2 and got["info"][5] > 0 and got["info"][6] == 0 and got["info"][7] == 0
    want = lba.local_ba_optimize(*args, N_SWITCH, 0)
    print("info", got["info"], want["info"], "vs oracle: poses %.3g points %.3g" % (np.abs(got["poses"] - want["poses"]).max(),
                                                                                     np.abs(got["points"] - want["points"]).max()))
    assert got["info"][2] == want["info"][4]
    assert np.allclose(got["info"][:2], want["info"][:2], rtol=1e-7)
    assert np.allclose(got["poses"], want["poses"], rtol=1e-7, atol=1e-8) and np.allclose(got["points"], want["points"], rtol=1e-7, atol=1e-8)
    host = ba.local_ba_optimize(*args, N_SWITCH, 0)   # beyond the Cholesky's size: local BA's host path
    print("vs local BA's host path: poses %.3g points %.3g" % (np.abs(got["poses"] - host["poses"]).max(), np.abs(got["points"] - host["points"]).max()))
    assert np.allclose(got["poses"], host["poses"], rtol=1e-9, atol=1e-10) and np.allclose(got["points"], host["points"], rtol=1e-9, atol=1e-10)
    with pytest.raises(OvsError) as e:
        ba.global_ba_optimize(*args, hm, hs, N_SWITCH, ba.SOLVER_CHOLESKY)
    assert e.value.status == -4


@pytest.mark.parametrize("also_fixed,n_free", [((), 258), ((130,), 257)])
def test_whole_call_with_a_second_lane_per_block_workgroup(oracle, also_fixed, n_free):
    """A ring of 259 keyframes, mono edges, three LM iterations: 258 free keyframes (keyframe 0 fixed), and 257 with keyframe 130 fixed as
    well (the fixed mask is no prefix, and the last workgroup of the lane-per-block kernels holds one lane). The bounds are those of the
    1026-unknown test between the same pairs. Beyond this size the suite compares the whole call with nothing."""
    from oracle import lba
    from openvslam_amd import ba
    d = dict(global_ba_ref.ring(259, 6000, 100))
    fixed = np.array(d["pose_fixed"], np.uint8)
    fixed[list(also_fixed)] = 1
    assert int((fixed == 0).sum()) == n_free and fixed[0] == 1
    hm, hs = ba.huber_deltas(0)
    args = (d["poses"], fixed, d["points"], d["edges"], d["cam"], None, 0.0)
    got = ba.global_ba_optimize(*args, hm, hs, N_SWITCH, ba.SOLVER_BY_SIZE)
    assert got["info"][4] == 2 and got["info"][5] > 16 * got["info"][3] and got["info"][6] == 0 and got["info"][7] == 0   # more than one chunk per solve
    want = lba.local_ba_optimize(*args, N_SWITCH, 0)
    print("info", got["info"], want["info"], "vs oracle: poses %.3g points %.3g" % (np.abs(got["poses"] - want["poses"]).max(),
                                                                                     np.abs(got["points"] - want["points"]).max()))
    assert got["info"][2] == want["info"][4]
    assert np.allclose(got["info"][:2], want["info"][:2], rtol=1e-7)
    assert np.allclose(got["poses"], want["poses"], rtol=1e-7, atol=1e-8) and np.allclose(got["points"], want["points"], rtol=1e-7, atol=1e-8)
    host = ba.local_ba_optimize(*args, N_SWITCH, 0)   # local BA's host path
    print("vs local BA's host path: poses %.3g points %.3g" % (np.abs(got["poses"] - host["poses"]).max(), np.abs(got["points"] - host["points"]).max()))
    assert np.allclose(got["poses"], host["poses"], rtol=1e-9, atol=1e-10) and np.allclose(got["points"], host["points"], rtol=1e-9, atol=1e-10)
    rows = np.flatnonzero(fixed)
    assert _same_bits(got["poses"][rows], np.asarray(d["poses"], np.float64)[rows])
    assert np.abs(got["poses"][fixed == 0] - np.asarray(d["poses"])[fixed == 0]).max() > 1e-3   # (the free ones move by far more than the bounds)


# ---- A6: Huber and edge kinds -----------------------------------------------------------------------------------------------------------
def _oracle_round(d, mono, st, bf, num_iter, robust):
    """One round of the oracle's Levenberg-Marquardt with the kernels on or off (local_ba_optimize always has them on in round 1)."""
    from oracle import binding as ob
    from oracle import lba
    poses = np.array(d["poses"], np.float64)
    T = [(lba._quat_to_rot(p[3:]), p[:3].copy()) for p in poses]
    st = np.ascontiguousarray(st if st is not None else np.zeros(0, ob.BA_EDGE_STEREO_DTYPE), ob.BA_EDGE_STEREO_DTYPE)
    G = lba._Graph(len(poses), len(d["points"]), d["pose_fixed"], np.ascontiguousarray(mono, ob.BA_EDGE_DTYPE), st, tuple(d["cam"]), bf, 1)
    T, X, chi0, chi1, n_iter, _, _ = G.run_round(T, np.array(d["points"], np.float64), num_iter, robust)
    P = poses.copy()
    for k in G.free:
        P[k, :3], P[k, 3:] = T[k][1], lba._rot_to_quat(T[k][0])
    return P, X, chi0, chi1, n_iter


@pytest.mark.parametrize("robust", [True, False])
@pytest.mark.parametrize("solver", [1, 2])
def test_mixed_edges_with_and_without_huber_against_the_oracle(oracle, robust, solver):
    from openvslam_amd import ba
    d, mono, st, bf = _scene(0.3)
    got = _global(d, mono, st, bf, solver, huber=None if robust else (0.0, 0.0))
    P, X, chi0, chi1, n_iter = _oracle_round(d, mono, st, bf, 10, robust)
    assert got["info"][2] == n_iter
    assert np.allclose(got["info"][:2], [chi0, chi1], rtol=1e-7)
    assert np.allclose(got["poses"], P, rtol=1e-7, atol=1e-8) and np.allclose(got["points"], X, rtol=1e-7, atol=1e-8)


@pytest.mark.parametrize("solver", [1, 2])
def test_equirect_entry_against_the_oracle(oracle, solver):
    from oracle import lba
    from openvslam_amd import ba
    from test_gpu_ba import _equirect_scene
    poses, fixed, pts, edges = _equirect_scene(11, n_pose=8, n_pt=1200, obs_per_pose=400, cols=3840, rows=1920)
    got = ba.global_ba_optimize_equirect(poses, fixed, pts, edges, 3840, 1920, ba.HUBER_2D, 10, solver)
    want = lba.local_ba_optimize_equirect(poses, fixed, pts, edges, 3840, 1920, 10, 0)
    assert got["info"][2] == want["info"][4] >= 2 and got["info"][4] == solver
    assert np.allclose(got["info"][:2], want["info"][:2], rtol=1e-7)
    assert np.allclose(got["poses"], want["poses"], rtol=1e-7, atol=1e-8) and np.allclose(got["points"], want["points"], rtol=1e-7, atol=1e-8)
    assert _same_bits(got["poses"][:3], poses[:3])
    from openvslam_amd._lib import OvsError
    with pytest.raises(OvsError) as e:
        ba.global_ba_optimize_equirect(poses, fixed, pts, edges, 0, 1920)
    assert e.value.status == -1


# ---- A7: the edges of the call ------------------------------------------------------------------------------------------------------------
def test_edges_of_the_call():
    from openvslam_amd import ba
    from openvslam_amd._lib import OvsError
    d, mono, st, bf = _scene(0.3)
    # every keyframe fixed: the landmarks alone move, on either solver setting (there is no system to solve)
    all_fixed = dict(d, pose_fixed=np.ones(len(d["poses"]), np.uint8))
    a = _global(all_fixed, mono, st, bf, ba.SOLVER_BY_SIZE)
    b = _global(all_fixed, mono, st, bf, ba.SOLVER_PCG)
    assert _same_bits(a["poses"], d["poses"]) and a["info"][1] < a["info"][0] and a["info"][4] == 1
    assert _same_bits(a["points"], b["points"]) and b["info"][5] == 0
    # no edges, no iterations, a stop flag that is set: the state keeps its bits
    for r in (ba.global_ba_optimize(d["poses"], d["pose_fixed"], d["points"], None, d["cam"], None, bf),
              _global(d, mono, st, bf, ba.SOLVER_PCG, num_iter=0),
              _global(d, mono, st, bf, ba.SOLVER_PCG, force_stop_flag=np.ones(1, np.uint8))):
        assert _same_bits(r["poses"], d["poses"]) and _same_bits(r["points"], d["points"]) and r["info"][2] == 0 and r["info"][3] == 0
    assert _global(d, mono, st, bf, ba.SOLVER_PCG, num_iter=0)["info"][0] > 0   # (the start's chi2 is still reported)
    # bad arguments
    for kw in (dict(solver=3), dict(solver=-1), dict(num_iter=-1), dict(huber=(-1.0, 0.0)), dict(huber=(0.0, float("nan"))), dict(huber=(float("inf"), 1.0))):
        with pytest.raises(OvsError) as e:
            _global(d, mono, st, bf, **dict(dict(solver=2), **kw))
        assert e.value.status == -1, kw
    bad = mono.copy()
    bad["pose_idx"][5] = len(d["poses"])
    with pytest.raises(OvsError) as e:
        _global(d, bad, st, bf, 2)
    assert e.value.status == -1
    # one keyframe beyond the capacity: refused by the plan, before anything is allocated (the arrays here could not even be indexed)
    n_over = ba.pcg_max_free() + 1
    assert ba.pcg_max_free() >= 512
    with pytest.raises(OvsError) as e:
        ba.global_ba_optimize(np.tile([0, 0, 0, 0, 0, 0, 1.0], (n_over, 1)), None, np.zeros((1, 3)), None, d["cam"], solver=ba.SOLVER_PCG)
    assert e.value.status == -4
    with pytest.raises(OvsError) as e:
        ba.global_ba_optimize(np.tile([0, 0, 0, 0, 0, 0, 1.0], (172, 1)), None, np.zeros((1, 3)), None, d["cam"], solver=ba.SOLVER_CHOLESKY)
    assert e.value.status == -4


def test_two_calls_and_two_threads_give_the_same_bits():
    from openvslam_amd import ba
    d, mono, st, bf = _scene(0.3)
    first = _global(d, mono, st, bf, ba.SOLVER_PCG)
    again = _global(d, mono, st, bf, ba.SOLVER_PCG)
    assert _same_bits(first["poses"], again["poses"]) and _same_bits(first["points"], again["points"]) and np.array_equal(first["info"], again["info"])
    out = [None, None]

    def work(i):
        out[i] = _global(d, mono, st, bf, ba.SOLVER_PCG)   # (a thread has its own work space and stream)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for r in out:
        assert r is not None and _same_bits(r["poses"], first["poses"]) and _same_bits(r["points"], first["points"])
        assert np.array_equal(r["info"], first["info"])


@pytest.mark.parametrize("name", ["ring24", "ring24_far"])
def test_lm_path_of_the_cpu_restatement(oracle, name):
    """The scene on which the restatement rejects trials: the device takes the same number of iterations and trials."""
    from openvslam_amd import ba
    d, want = global_ba_ref.reference(name)
    hm, hs = ba.huber_deltas(0)
    got = ba.global_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], None, 0.0, hm, hs, 10, ba.SOLVER_PCG)
    print("device", got["info"], "restatement", want["info"])
    assert got["info"][2] == want["info"][2] and got["info"][3] == want["info"][3] and got["info"][7] == want["info"][5]
    if name == "ring24_far":
        # counts only: after ten iterations this start is still at a chi2 of 1e6, far from a minimum, and a path that is not converging has
        # no state bound to hold two summation orders to (found: chi2 equal to 2.8e-7 relative, 247 against 248 solver iterations)
        assert got["info"][3] > got["info"][2]
        return
    assert np.allclose(got["info"][:2], want["info"][:2], rtol=1e-7)
    assert np.allclose(got["poses"], want["poses"], rtol=1e-7, atol=1e-8) and np.allclose(got["points"], want["points"], rtol=1e-7, atol=1e-8)


# ---- A8: the class layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 5])
def test_python_class_on_a_saved_map(tmp_path, lead):
    from openvslam_amd import ba, io, synth
    db0, d = synth.synth_map(n_pose=8, n_pt=900, obs_per_pose=300, seed=5, stereo_frac=0.3, pose_noise=0.03, point_noise=0.03)
    path = str(tmp_path / "map.msg")
    io.save_map_database(path, db0)
    db = io.load_map_database(path)
    db.keyframes[6].will_be_erased = True
    some_lm = sorted(db.landmarks)[3]
    db.landmarks[some_lm].will_be_erased = True
    prob = io.global_ba_problem(db)
    hm, hs = ba.huber_deltas(prob["setup_type"])
    want = ba.global_ba_optimize(prob["poses"], prob["pose_fixed"], prob["points"], prob["mono"], prob["cam"], prob["stereo"], prob["focal_x_baseline"],
                                 hm, hs, 10)
    assert want["info"][1] < want["info"][0] and 6 not in prob["keyfrm_ids"] and some_lm not in prob["lm_ids"]
    before = {k: (kf.trans_cw.copy(), kf.rot_cw.copy()) for k, kf in db.keyframes.items()}
    before_lm = {j: lm.pos_w.copy() for j, lm in db.landmarks.items()}
    adj = ba.global_bundle_adjuster(db, 10, True)
    adj.optimize(lead)
    assert np.array_equal(adj.info, want["info"])
    for i, k in enumerate(prob["keyfrm_ids"]):
        kf = db.keyframes[k]
        if lead == 0:
            assert _same_bits(kf.trans_cw, want["poses"][i, :3]) and _same_bits(kf.rot_cw, want["poses"][i, 3:])
        else:
            assert _same_bits(kf.trans_cw, before[k][0]) and _same_bits(kf.rot_cw, before[k][1]) and kf.loop_BA_identifier == lead
            assert _same_bits(kf.trans_cw_after_loop_BA, want["poses"][i, :3]) and _same_bits(kf.rot_cw_after_loop_BA, want["poses"][i, 3:])
    assert _same_bits(want["poses"][0], prob["poses"][0])   # keyframe 0 is fixed: its bits stay
    for i, j in enumerate(prob["lm_ids"]):
        lm = db.landmarks[j]
        if lead == 0:
            assert _same_bits(lm.pos_w, want["points"][i])
        else:
            assert _same_bits(lm.pos_w, before_lm[j]) and _same_bits(lm.pos_w_after_global_BA, want["points"][i]) and lm.loop_BA_identifier == lead
    # what is to be erased is not touched
    assert _same_bits(db.keyframes[6].trans_cw, before[6][0]) and db.keyframes[6].loop_BA_identifier == 0
    assert _same_bits(db.landmarks[some_lm].pos_w, before_lm[some_lm]) and db.landmarks[some_lm].pos_w_after_global_BA is None
    # a stop flag that is set leaves the map as it is
    db2 = io.load_map_database(path)
    ba.global_bundle_adjuster(db2).optimize(lead, np.ones(1, np.uint8))
    for k, kf in db2.keyframes.items():
        assert _same_bits(kf.trans_cw, db0.keyframes[k].trans_cw) and kf.loop_BA_identifier == 0


def _globalba_shim():
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "openvslam_amd", "cpp"), "test_globalba_shim"])
    return os.path.join(root, "openvslam_amd", "cpp", "test_globalba_shim")


def test_cpp_class_on_a_saved_map(tmp_path):
    """map.msg -> io::map_database_io -> optimize::global_bundle_adjuster::optimize == the Python path on the same file, both write-back
    branches. The two flatten a landmark's observations in different orders (a std::map keyed by pointer against ascending keyframe id), so
    the block sums are associated differently: states agree to 1e-6, test_map_io.py's bound for the local adjuster's two layers. Under
    injected failures (calls that REPORT failure) the map is left as it was loaded."""
    import re
    import subprocess
    from openvslam_amd import ba, io, synth
    db0, d = synth.synth_map(n_pose=8, n_pt=900, obs_per_pose=300, seed=5, stereo_frac=0.3, pose_noise=0.03, point_noise=0.03)
    path = str(tmp_path / "map.msg")
    io.save_map_database(path, db0)
    db = io.load_map_database(path)
    ba.global_bundle_adjuster(db, 10, True).optimize(0)
    nk, nl = len(db.keyframes), len(db.landmarks)

    def run(lead, *extra):
        out = str(tmp_path / "out.bin")
        r = subprocess.run([_globalba_shim(), path, str(lead), out] + list(extra), capture_output=True, text=True, check=True)
        raw = np.fromfile(out, np.float64)
        assert len(raw) == 33 * nk + 7 * nl
        return r.stdout, raw[:33 * nk].reshape(nk, 33), raw[33 * nk:].reshape(nl, 7)

    def pose_of(kf):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = ba.quat_to_rot(kf.rot_cw), kf.trans_cw
        return T

    want_T = np.stack([pose_of(db.keyframes[k]) for k in sorted(db.keyframes)])
    want_X = np.stack([db.landmarks[j].pos_w for j in sorted(db.landmarks)])
    start_T = np.stack([pose_of(db0.keyframes[k]) for k in sorted(db0.keyframes)])
    start_X = np.stack([db0.landmarks[j].pos_w for j in sorted(db0.landmarks)])
    assert np.abs(want_X - start_X).max() > 1e-3   # (the optimisation moves the map by far more than the bounds below)
    # lead 0: straight into the map
    _, K, Lm = run(0)
    assert np.allclose(K[:, :16].reshape(nk, 4, 4), want_T, rtol=1e-6, atol=1e-6) and np.allclose(Lm[:, :3], want_X, rtol=1e-6, atol=1e-6)
    assert not K[:, 16:].any() and not Lm[:, 3:].any()
    loaded = run(0, "fail")[1]   # (a run that leaves the map untouched dumps the poses as the loader made them)
    assert _same_bits(K[0, :16], loaded[0, :16])   # keyframe 0 is fixed: its matrix keeps its bits
    # any other lead: the map keeps its state, the result waits in the after-loop-BA members
    _, K, Lm = run(5)
    assert np.allclose(K[:, :16].reshape(nk, 4, 4), start_T, rtol=0, atol=1e-15) and np.array_equal(Lm[:, :3], start_X)
    assert np.allclose(K[:, 16:32].reshape(nk, 4, 4), want_T, rtol=1e-6, atol=1e-6) and np.allclose(Lm[:, 3:6], want_X, rtol=1e-6, atol=1e-6)
    assert (K[:, 32] == 5).all() and (Lm[:, 6] == 5).all()
    assert _same_bits(K[0, 16:32], loaded[0, :16]) and _same_bits(K[:, :16], loaded[:, :16])
    # a device that reports failure on every call: one retry, then the map untouched
    text, K, Lm = run(0, "fail")
    assert int(re.search(r"degraded calls (\d+)", text).group(1)) == 1
    assert np.allclose(K[:, :16].reshape(nk, 4, 4), start_T, rtol=0, atol=1e-15) and np.array_equal(Lm[:, :3], start_X)
    assert not K[:, 16:].any() and not Lm[:, 3:].any()
