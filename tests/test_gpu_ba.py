"""GPU parity of the local-BA linearisation (config 5: 50 keyframes x 2000 observations, 20 000 landmarks, fp64).
Stated tolerances (BASELINE north_star asks for them): per-edge Hpl blocks bit-exact; sums (Hpp, bp, Hll, bl, chi2) within
1e-12 relative on one GPU (atomic summation order), the multi-rank path is covered on CPU with 1e-10."""
import os

import numpy as np
import pytest

from openvslam_amd.synth import synth_local_ba

pytestmark = pytest.mark.gpu


def _check(got, want, rtol):
    assert np.array_equal(got["Hpl"], want["Hpl"])
    for k in ("Hpp", "bp", "Hll", "bl", "chi2"):
        scale = np.abs(want[k]).max()
        assert np.allclose(got[k], want[k], rtol=rtol, atol=rtol * scale), k


@pytest.mark.parametrize("huber", [True, False])
def test_config5_full_size(oracle, huber):
    from openvslam_amd import ba
    d = synth_local_ba(seed=0)
    delta = d["huber_delta"] if huber else 0.0
    got = ba.linearize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], delta)
    want = oracle.ba_linearize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], delta)
    _check(got, want, 1e-12)
    assert len(d["edges"]) == 100000


def test_unsorted_edges_and_no_fixed(oracle):
    from openvslam_amd import ba
    d = synth_local_ba(n_pose=9, n_pt=700, obs_per_pose=333, seed=7, pose_noise=0.05, point_noise=0.05)
    rng = np.random.default_rng(0)
    e = d["edges"][rng.permutation(len(d["edges"]))]           # waves see mixed poses: per-lane atomic path
    got = ba.linearize(d["poses"], None, d["points"], e, d["cam"], d["huber_delta"])
    want = oracle.ba_linearize(d["poses"], None, d["points"], e, d["cam"], d["huber_delta"])
    _check(got, want, 1e-12)


def test_device_linearizer_single_rank(oracle):
    import torch
    from openvslam_amd import ba
    d = synth_local_ba(n_pose=12, n_pt=2000, obs_per_pose=500, seed=9)
    lin = ba.local_ba_linearizer(d["cam"], d["huber_delta"])
    out = lin.linearize(torch.from_numpy(d["poses"]).cuda(), torch.from_numpy(d["pose_fixed"]).cuda(), torch.from_numpy(d["points"]).cuda(),
                        torch.from_numpy(d["edges"].view(np.uint8)).cuda())
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    want = oracle.ba_linearize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], d["huber_delta"])
    _check(got, want, 1e-12)


def _stereo_edges(d, bf, frac=1.0, seed=0):
    """Stereo observations for a synth_local_ba scene: u_r = u - bf / z + N(0, 1)."""
    from openvslam_amd import ba
    rng = np.random.default_rng(seed)
    e = d["edges"]
    keep = rng.random(len(e)) < frac
    e = e[keep]
    se = np.zeros(len(e), ba.EDGE_STEREO_DTYPE)
    for k in ("pose_idx", "point_idx", "obs_x", "obs_y", "inv_sigma_sq"):
        se[k] = e[k]
    # depth of each point in its keyframe
    from openvslam_amd.ba import quat_to_rot
    z = np.empty(len(e))
    for p in np.unique(e["pose_idx"]):
        R = quat_to_rot(d["poses_true"][p, 3:])
        sel = e["pose_idx"] == p
        z[sel] = (d["points_true"][e["point_idx"][sel]] @ R.T + d["poses_true"][p, :3])[:, 2]
    se["obs_x_right"] = e["obs_x"] - bf / z + rng.normal(0, 1, len(e))
    return se, d["edges"][~keep]


@pytest.mark.parametrize("huber", [True, False])
def test_stereo_edges(oracle, huber):
    from openvslam_amd import ba
    d = synth_local_ba(n_pose=20, n_pt=5000, obs_per_pose=1500, seed=3, pose_noise=0.02, point_noise=0.02)
    bf = 0.12 * d["cam"][0]
    se, _ = _stereo_edges(d, bf)
    delta = float(np.sqrt(7.815)) if huber else 0.0
    got = ba.linearize_stereo(d["poses"], d["pose_fixed"], d["points"], se, d["cam"], bf, delta)
    want = oracle.ba_linearize_stereo(d["poses"], d["pose_fixed"], d["points"], se, d["cam"], bf, delta)
    _check(got, want, 1e-12)
    assert len(se) == 30000 and want["chi2"][0] > 0


def _equirect_scene(seed, n_pose=20, n_pt=5000, obs_per_pose=1500, cols=1920, rows=960):
    """Landmarks on a shell around the rig, equirectangular observations with 1 px noise, perturbed initial state."""
    from openvslam_amd import ba
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n_pt, 3))
    pts *= (rng.uniform(3.0, 9.0, n_pt) / np.linalg.norm(pts, axis=1))[:, None]
    poses = np.zeros((n_pose, 7))
    for i in range(n_pose):
        q = np.concatenate([rng.normal(0, 0.1, 3), [1.0]])
        poses[i, 3:] = q / np.linalg.norm(q)
        poses[i, :3] = rng.normal(0, 0.4, 3)
    edges = np.zeros(n_pose * obs_per_pose, ba.EDGE_DTYPE)
    for i in range(n_pose):
        sel = rng.choice(n_pt, obs_per_pose, replace=False)
        p = pts[sel] @ ba.quat_to_rot(poses[i, 3:]).T + poses[i, :3]
        u = cols * (0.5 + np.arctan2(p[:, 0], p[:, 2]) / (2 * np.pi))
        v = rows * (0.5 + np.arcsin(p[:, 1] / np.linalg.norm(p, axis=1)) / np.pi)
        e = edges[i * obs_per_pose:(i + 1) * obs_per_pose]
        e["pose_idx"], e["point_idx"] = i, sel
        e["obs_x"], e["obs_y"] = u + rng.normal(0, 1, obs_per_pose), v + rng.normal(0, 1, obs_per_pose)
        e["inv_sigma_sq"] = 1.0 / 1.2 ** (2 * rng.integers(0, 8, obs_per_pose))
    noisy_pts = pts + rng.normal(0, 0.02, pts.shape)
    noisy = poses.copy()
    noisy[:, :3] += rng.normal(0, 0.02, (n_pose, 3))
    fixed = np.zeros(n_pose, np.uint8)
    fixed[:3] = 1
    return noisy, fixed, noisy_pts, edges


@pytest.mark.parametrize("huber", [True, False])
def test_equirectangular_edges(oracle, huber):
    """atan2 / asin come from two maths libraries (ocml on the GPU, glibc in the oracle), so the residuals and with Huber the
    weights can differ in the last place: every block within 1e-11 relative; without Huber the Jacobian-only Hpl blocks are exact."""
    from openvslam_amd import ba
    poses, fixed, pts, edges = _equirect_scene(5)
    delta = float(np.sqrt(5.991)) if huber else 0.0
    got = ba.linearize_equirect(poses, fixed, pts, edges, 1920, 960, delta)
    want = oracle.ba_linearize_equirect(poses, fixed, pts, edges, 1920, 960, delta)
    if not huber:
        assert np.array_equal(got["Hpl"], want["Hpl"])
    for k in ("Hpl", "Hpp", "bp", "Hll", "bl", "chi2"):
        scale = np.abs(want[k]).max()
        assert np.allclose(got[k], want[k], rtol=1e-11, atol=1e-11 * scale), k
    assert want["chi2"][0] > 0 and np.abs(want["Hpl"]).max() > 0
    assert ba.linearize_equirect is not None


def test_equirectangular_rejects_bad_image_size():
    from openvslam_amd import ba
    poses, fixed, pts, edges = _equirect_scene(6, n_pose=2, n_pt=50, obs_per_pose=20)
    with pytest.raises(RuntimeError):
        ba.linearize_equirect(poses, fixed, pts, edges, 0, 960, 0.0)


@pytest.mark.parametrize("stereo_frac,n_pose,n_pt,obs", [(0.0, 10, 1500, 500), (0.3, 10, 1500, 500), (1.0, 6, 800, 300), (0.0, 50, 20000, 2000)])
def test_local_ba_optimize(oracle, stereo_frac, n_pose, n_pt, obs):
    """B4: both rounds of local_bundle_adjuster::optimize against the numpy / C oracle. The two sides sum the blocks in different
    orders (atomics vs sequential) and the host solves differ in operation order, so states agree to 1e-7 relative after 15
    Levenberg-Marquardt iterations; iteration counts and the outlier flags must be identical apart from observations whose chi2 sits
    within 1e-6 of the gate."""
    from oracle import lba
    from openvslam_amd import ba
    from test_ba import _lba_scene
    d, mono, st, bf, _, _ = _lba_scene(3, n_pose=n_pose, n_pt=n_pt, obs_per_pose=obs, stereo_frac=stereo_frac)
    got = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], st, bf)
    want = lba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], st, bf)
    assert np.array_equal(got["info"][4:], want["info"][4:]) and want["info"][4] >= 3
    assert np.allclose(got["info"][:4], want["info"][:4], rtol=1e-7)
    assert np.allclose(got["poses"], want["poses"], rtol=1e-7, atol=1e-8)
    assert np.allclose(got["points"], want["points"], rtol=1e-7, atol=1e-8)
    for k in ("mono_outlier", "stereo_outlier"):
        assert (got[k] != want[k]).sum() <= max(1, len(want[k]) // 5000), k
    fixed = d["pose_fixed"].astype(bool)
    assert np.array_equal(got["poses"][fixed], d["poses"][fixed])


@pytest.mark.parametrize("n_pose,n_pt,obs,outliers,polar", [(8, 1200, 400, 0.0, True), (12, 3000, 800, 0.03, False), (12, 3000, 800, 0.03, True),
                                                             (4, 300, 150, 0.1, False)])
def test_local_ba_optimize_equirect(oracle, n_pose, n_pt, obs, outliers, polar):
    """Both rounds of local_bundle_adjuster::optimize over equirectangular_reproj_edge (BASELINE configs[3] camera model) against the oracle:
    same iteration counts, states within 1e-7, outlier flags identical apart from observations on the chi2 gate. Bearings cover the whole
    sphere, i.e. include the +-180 degree seam and both poles."""
    from oracle import lba
    from openvslam_amd import ba
    poses, fixed, pts, edges = _equirect_scene(11, n_pose=n_pose, n_pt=n_pt, obs_per_pose=obs, cols=3840, rows=1920)
    if not polar:   # keep the landmarks below 72 degrees of latitude: the edge's Jacobian grows like 1 / cos(latitude)^2
        lat_ok = np.abs(pts[:, 1]) / np.linalg.norm(pts, axis=1) < 0.95
        edges = edges[lat_ok[edges["point_idx"]]]
    rng = np.random.default_rng(5)
    bad = rng.random(len(edges)) < outliers
    edges["obs_x"][bad] += rng.uniform(30, 200, int(bad.sum()))
    got = ba.local_ba_optimize_equirect(poses, fixed, pts, edges, 3840, 1920)
    want = lba.local_ba_optimize_equirect(poses, fixed, pts, edges, 3840, 1920)
    assert np.array_equal(got["info"][4:], want["info"][4:]) and want["info"][4] >= 2
    # stated tolerance: 1e-7 as for the perspective cases. With landmarks near the poles AND planted outliers the normal equations are
    # dominated by a handful of 1 / cos(latitude)^2 Jacobian entries (condition ~1e10): the different association of the block sums (tree vs
    # sequential) then shows at 2e-6 in chi2 and 2e-5 in the worst keyframe's translation -- upstream's own solve has the same conditioning
    # Round 4 (device solve of the reduced camera system, blocks of it summed per keyframe pair on the device): every change of the summation
    # order moves THIS case by another 1e-4 (8e-5, then 2e-4 in that keyframe's translation) while the cost stays equal to 1e-4 and the other
    # three cases hold 1e-7 -- the minimum is flat along the directions those Jacobian entries leave undetermined. Stated for this case:
    # chi2 to 1e-4, states to 1e-3 (ORACLE_SPEC rule 25).
    tol = 1e-4 if (polar and outliers) else 1e-7
    stol = 1e-3 if (polar and outliers) else 1e-7
    assert np.allclose(got["info"][:4], want["info"][:4], rtol=tol), (got["info"], want["info"])
    assert np.allclose(got["poses"], want["poses"], rtol=stol, atol=stol / 10), np.abs(got["poses"] - want["poses"]).max()
    assert np.allclose(got["points"], want["points"], rtol=stol, atol=stol / 10), np.abs(got["points"] - want["points"]).max()
    assert (got["mono_outlier"] != want["mono_outlier"]).sum() <= max(1, len(edges) // 5000)
    if polar and outliers:
        # regression guard: with the HOST solve of the reduced camera system -- the more accurate of the two forms, ORACLE_SPEC
        # "Tolerances of the two solver forms" -- BOTH forms are held to absolute bounds here (keyframe states 5e-4, points 1e-2). Measured in round 5: device 8.1e-5 / 1.7e-3, host 1.4e-4 /
        # 2.9e-3 -- on this case the minimum is flat along the directions the polar Jacobian entries leave undetermined and neither form is
        # "the accurate one"; 1e-4 was the bound of round 3, before the Schur blocks were summed per keyframe pair on the device
        try:
            ba.local_ba_set_solver("host")
            hst = ba.local_ba_optimize_equirect(poses, fixed, pts, edges, 3840, 1920)
        finally:
            ba.local_ba_set_solver("device")
        assert np.array_equal(hst["info"][4:], want["info"][4:])
        dev_p, dev_x = np.abs(got["poses"] - want["poses"]).max(), np.abs(got["points"] - want["points"]).max()
        hst_p, hst_x = np.abs(hst["poses"] - want["poses"]).max(), np.abs(hst["points"] - want["points"]).max()
        print("equirect polar + outliers: max |d pose| device %.2e host %.2e, max |d point| device %.2e host %.2e" % (dev_p, hst_p, dev_x, hst_x))
        assert hst_p < 5e-4 and hst_x < 1e-2 and dev_p < 5e-4 and dev_x < 1e-2, (dev_p, hst_p, dev_x, hst_x)
    if outliers and n_pose >= 8:   # (the 4-keyframe scene observes many landmarks once: those absorb a planted outlier)
        assert (want["mono_outlier"] == bad).mean() > 0.95
    assert np.array_equal(got["poses"][fixed.astype(bool)], poses[fixed.astype(bool)])
    assert want["info"][3] < want["info"][0]


def test_graph_equirect_matches_oracle(oracle):
    """ovs_ba_graph_create_equirect + linearize: Hll / bl / Hpl bit-equal to the oracle's sequential sums (same asin / atan2 on both sides)."""
    import ctypes as C
    import torch
    from openvslam_amd import _lib, ba
    poses, fixed, pts, edges = _equirect_scene(12, n_pose=6, n_pt=900, obs_per_pose=300, cols=3840, rows=1920)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.ovs_ba_graph_create_equirect(0, len(poses), fixed.ctypes.data_as(C.c_void_p), len(pts), edges.ctypes.data_as(C.c_void_p), len(edges),
                                              3840, 1920, C.byref(h)), "ovs_ba_graph_create_equirect")
    try:
        dp, dx = torch.from_numpy(poses).cuda(), torch.from_numpy(pts).cuda()
        o = dict(Hpp=torch.zeros((len(poses), 6, 6), dtype=torch.float64, device="cuda"), bp=torch.zeros((len(poses), 6), dtype=torch.float64, device="cuda"),
                 Hll=torch.zeros((len(pts), 3, 3), dtype=torch.float64, device="cuda"), bl=torch.zeros((len(pts), 3), dtype=torch.float64, device="cuda"),
                 Hpl=torch.zeros((len(edges), 6, 3), dtype=torch.float64, device="cuda"), chi2=torch.zeros(3, dtype=torch.float64, device="cuda"))
        delta = float(np.sqrt(np.float32(5.99146)))
        _lib.check(L.ovs_ba_graph_linearize_dev(h, dp.data_ptr(), dx.data_ptr(), delta, 0.0, o["Hpp"].data_ptr(), o["bp"].data_ptr(), o["Hll"].data_ptr(),
                                                o["bl"].data_ptr(), o["Hpl"].data_ptr(), o["chi2"].data_ptr(), None), "linearize")
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items()}
    finally:
        L.ovs_ba_graph_destroy(h)
    want = oracle.ba_linearize_equirect(poses, fixed, pts, edges, 3840, 1920, delta)
    for k in ("Hll", "bl", "Hpl"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("Hpp", "bp"):
        assert np.allclose(got[k], want[k], rtol=1e-12, atol=1e-12 * np.abs(want[k]).max()), k
    assert np.allclose(got["chi2"][:2], want["chi2"], rtol=1e-12)


_EDGE_MODEL_SCENES = {}


def _edge_model_scene(kind):
    """The smallest scene that crosses every partition boundary of k_linearize2: 3 keyframes, 600 landmarks. Keyframe 0 observes all 600 (one
    full 512-entry chunk and a partial one), keyframe 1 observes 257 (one entry over a half chunk), keyframe 2 observes 70 and is fixed;
    landmark 0 is observed by all three. kind: "mono" | "stereo" (a third of the edges stereo) | "equirect".
    Returns (poses, fixed, points, mono edges ordered by keyframe, stereo edges ordered by keyframe, cam or None, bf)."""
    if kind in _EDGE_MODEL_SCENES:
        return _EDGE_MODEL_SCENES[kind]
    from openvslam_amd import ba
    if kind == "equirect":
        poses, _, pts, e = _equirect_scene(31, n_pose=3, n_pt=600, obs_per_pose=600)
        d, cam = None, None
    else:
        d = synth_local_ba(n_pose=3, n_pt=600, obs_per_pose=600, seed=31, pose_noise=0.02, point_noise=0.02, n_fixed=0)
        poses, pts, e, cam = d["poses"], d["points"], d["edges"], d["cam"]
    rng = np.random.default_rng(32)
    keep = np.zeros(len(e), bool)
    for k, n in ((0, 600), (1, 257), (2, 70)):
        idx = np.flatnonzero(e["pose_idx"] == k)
        idx = idx[np.argsort(e["point_idx"][idx], kind="stable")]
        keep[idx[0]] = True                                  # landmark 0
        keep[rng.choice(idx[1:], n - 1, replace=False)] = True
    e = e[keep]
    e = np.ascontiguousarray(e[np.lexsort((e["point_idx"], e["pose_idx"]))])
    assert np.bincount(e["pose_idx"]).tolist() == [600, 257, 70] and (e["point_idx"] == 0).sum() == 3
    if kind != "equirect":   # gross outliers for the chi-square gates (as test_ba._lba_scene plants them)
        bad = rng.random(len(e)) < 0.04
        e["obs_x"][bad] += rng.choice([-1, 1], int(bad.sum())) * rng.uniform(15, 60, int(bad.sum()))
    st, bf = np.zeros(0, ba.EDGE_STEREO_DTYPE), 0.0
    if kind == "stereo":
        bf = 0.12 * cam[0]
        st, e = _stereo_edges(dict(d, edges=e), bf, frac=1.0 / 3.0, seed=33)
        e = np.ascontiguousarray(e)
        assert len(st) > 250 and len(e) > 550
    fixed = np.array([0, 0, 1], np.uint8)
    _EDGE_MODEL_SCENES[kind] = (poses, fixed, pts, e, st, cam, bf)
    return _EDGE_MODEL_SCENES[kind]


def _graph_blocks(kind, poses, fixed, pts, mono, st, cam, bf, hm, hs):
    """One linearisation through the graph path (k_linearize2): dict of numpy blocks, Hpl in edge order (mono, then stereo)."""
    import ctypes as C
    import torch
    from openvslam_amd import _lib, ba
    P, X = torch.from_numpy(poses).cuda(), torch.from_numpy(pts).cuda()
    if kind != "equirect":
        g = ba.graph(len(poses), fixed, len(pts), mono, cam, st if len(st) else None, bf)
        out = g.linearize_dev(P, X, hm, hs)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy().copy() for k, t in ba.graph.views(out, g.n_pose, g.n_pt, g.n_edge).items()}
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.ovs_ba_graph_create_equirect(0, len(poses), fixed.ctypes.data_as(C.c_void_p), len(pts), mono.ctypes.data_as(C.c_void_p), len(mono),
                                              1920, 960, C.byref(h)), "ovs_ba_graph_create_equirect")
    try:
        o = dict(Hpp=torch.zeros((len(poses), 6, 6), dtype=torch.float64, device="cuda"), bp=torch.zeros((len(poses), 6), dtype=torch.float64, device="cuda"),
                 Hll=torch.zeros((len(pts), 3, 3), dtype=torch.float64, device="cuda"), bl=torch.zeros((len(pts), 3), dtype=torch.float64, device="cuda"),
                 Hpl=torch.zeros((len(mono), 6, 3), dtype=torch.float64, device="cuda"), chi2=torch.zeros(3, dtype=torch.float64, device="cuda"))
        _lib.check(L.ovs_ba_graph_linearize_dev(h, P.data_ptr(), X.data_ptr(), hm, 0.0, o["Hpp"].data_ptr(), o["bp"].data_ptr(), o["Hll"].data_ptr(),
                                                o["bl"].data_ptr(), o["Hpl"].data_ptr(), o["chi2"].data_ptr(), None), "linearize")
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items()}
        got["chi2"] = got["chi2"][:2]
        return got
    finally:
        L.ovs_ba_graph_destroy(h)


@pytest.mark.parametrize("huber", [True, False])
@pytest.mark.parametrize("kind", ["mono", "stereo", "equirect"])
def test_edge_model_call_sites_agree_per_edge(oracle, kind, huber):
    """The edge model has one definition (ba_edge.h) and four call sites: k_ba_linearize<2|3>, both sides of k_linearize2 and k_edge_chi2 (the
    last one: test_edge_model_chi2_gates_match_oracle). Per edge they and the oracle must give the same bits, with the edges ordered by keyframe
    (the wave-contiguous Hpl store) and shuffled (the per-lane store): Hpl equal between ovs_ba_linearize*, the graph and the oracle; the
    graph's Hll / bl equal to the oracle's sequential sums; Hpp / bp / chi2 (tree sums) at 1e-13 as in
    test_graph_linearize_is_deterministic_and_matches_oracle."""
    from oracle import lba
    from openvslam_amd import ba
    poses, fixed, pts, mono0, st0, cam, bf = _edge_model_scene(kind)
    hm = (lba.SQRT_CHI2_MONO if huber else 0.0)
    hs = (lba.SQRT_CHI2_STEREO if huber else 0.0)
    for shuffled in (False, True):
        mono, st = mono0, st0
        if shuffled:
            rng = np.random.default_rng(34)
            mono = np.ascontiguousarray(mono0[rng.permutation(len(mono0))])
            st = np.ascontiguousarray(st0[rng.permutation(len(st0))])
        if kind == "equirect":
            want = oracle.ba_linearize_equirect(poses, fixed, pts, mono, 1920, 960, hm)
            flat = ba.linearize_equirect(poses, fixed, pts, mono, 1920, 960, hm)["Hpl"]
        else:
            want = oracle.ba_linearize(poses, fixed, pts, mono, cam, hm)
            flat = ba.linearize(poses, fixed, pts, mono, cam, hm)["Hpl"]
            if len(st):
                s = oracle.ba_linearize_stereo(poses, fixed, pts, st, cam, bf, hs)
                for k in ("Hpp", "bp", "Hll", "bl", "chi2"):
                    want[k] = want[k] + s[k]
                want["Hpl"] = np.concatenate([want["Hpl"], s["Hpl"]])
                flat = np.concatenate([flat, ba.linearize_stereo(poses, fixed, pts, st, cam, bf, hs)["Hpl"]])
        got = _graph_blocks(kind, poses, fixed, pts, mono, st, cam, bf, hm, hs)
        assert np.abs(want["Hpl"]).max() > 0 and want["chi2"][0] > 0
        assert np.array_equal(flat, want["Hpl"]), shuffled
        assert np.array_equal(got["Hpl"], want["Hpl"]), shuffled
        for k in ("Hll", "bl"):
            assert np.array_equal(got[k], want[k]), (k, shuffled)
        for k in ("Hpp", "bp", "chi2"):
            scale = np.abs(want[k]).max()
            assert np.allclose(got[k][:len(want[k])], want[k], rtol=1e-13, atol=1e-13 * scale), (k, shuffled)


def test_edge_model_chi2_gates_match_oracle(oracle):
    """k_edge_chi2's use of the edge model: ovs_local_ba_optimize on the perspective scenes of test_edge_model_call_sites_agree_per_edge gives
    the oracle's iteration counts and outlier flags (the tolerances of test_local_ba_optimize)."""
    from oracle import lba
    from openvslam_amd import ba
    for kind in ("mono", "stereo"):
        poses, fixed, pts, mono, st, cam, bf = _edge_model_scene(kind)
        got = ba.local_ba_optimize(poses, fixed, pts, mono, cam, st, bf)
        want = lba.local_ba_optimize(poses, fixed, pts, mono, cam, st, bf)
        assert np.array_equal(got["info"][4:], want["info"][4:]) and want["info"][4] >= 1, kind
        assert np.allclose(got["info"][:4], want["info"][:4], rtol=1e-7), kind
        assert np.allclose(got["poses"], want["poses"], rtol=1e-7, atol=1e-8), kind
        assert np.allclose(got["points"], want["points"], rtol=1e-7, atol=1e-8), kind
        for k in ("mono_outlier", "stereo_outlier"):
            assert (got[k] != want[k]).sum() <= max(1, len(want[k]) // 5000), (kind, k)
        assert np.array_equal(got["poses"][2], poses[2])


def test_local_ba_force_stop_and_bad_args():
    from openvslam_amd import ba
    from test_ba import _lba_scene
    d, mono, st, bf, _, _ = _lba_scene(5, n_pose=6, n_pt=600, obs_per_pose=250)
    stop = np.ones(1, np.uint8)     # raised before the call: no iteration runs, the state comes back unchanged
    r = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], force_stop_flag=stop)
    assert r["info"][4] == 0 and r["info"][5] == 0
    assert np.allclose(r["poses"], d["poses"], rtol=0, atol=1e-12) and np.array_equal(r["points"], d["points"])
    bad = mono.copy()
    bad["point_idx"][0] = 10 ** 6
    with pytest.raises(RuntimeError):
        ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], bad, d["cam"])
    # one keyframe with two edges to one landmark (upstream's landmark::add_observation never produces it; the reduced system's pair
    # lists would miss the cross terms): refused at graph creation, with the pair named in ovs_last_error
    dup = np.concatenate([mono, mono[3:4]])
    with pytest.raises(RuntimeError, match="two edges to landmark"):
        ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], dup, d["cam"])


@pytest.mark.parametrize("stereo_frac", [0.0, 0.35])
def test_graph_linearize_is_deterministic_and_matches_oracle(oracle, stereo_frac):
    """The atomics-free graph path (round 2): Hll | bl | Hpl BIT-identical to the oracle (one lane per landmark adds its edges in the
    oracle's order), Hpp | bp | chi2 within 1e-13 (fixed-shape tree vs sequential sum), and two runs give identical bits."""
    import torch
    from oracle import lba
    from openvslam_amd import ba
    from test_ba import _lba_scene
    d, mono, st, bf, _, _ = _lba_scene(21, n_pose=12, n_pt=3000, obs_per_pose=700, stereo_frac=stereo_frac)
    hm, hs = lba.SQRT_CHI2_MONO, lba.SQRT_CHI2_STEREO
    g = ba.graph(len(d["poses"]), d["pose_fixed"], len(d["points"]), mono, d["cam"], st, bf)
    P, X = torch.from_numpy(d["poses"]).cuda(), torch.from_numpy(d["points"]).cuda()
    runs = []
    for _ in range(2):
        out = g.linearize_dev(P, X, hm, hs)
        torch.cuda.synchronize()
        v = ba.graph.views(out, g.n_pose, g.n_pt, g.n_edge)
        runs.append({k: t.cpu().numpy().copy() for k, t in v.items()})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k            # bit-reproducible
    want = oracle.ba_linearize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], hm)
    if len(st):
        s = oracle.ba_linearize_stereo(d["poses"], d["pose_fixed"], d["points"], st, d["cam"], bf, hs)
        for k in ("Hpp", "bp", "Hll", "bl", "chi2"):
            want[k] = want[k] + s[k]
        want["Hpl"] = np.concatenate([want["Hpl"], s["Hpl"]])
    got = runs[0]
    for k in ("Hpl", "Hll", "bl"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("Hpp", "bp", "chi2"):
        scale = np.abs(want[k]).max()
        assert np.allclose(got[k], want[k], rtol=1e-13, atol=1e-13 * scale), k
    free = d["pose_fixed"] == 0
    md = max(np.abs(np.einsum("kii->ki", want["Hpp"][free])).max(), np.abs(np.einsum("kii->ki", want["Hll"])).max())
    assert np.isclose(got["max_diag"][0], md, rtol=1e-13)


def test_graph_backend_under_nccl_group(oracle):
    """The HIP backend and a collective in ONE process group: a 1-rank nccl (RCCL) group drives local_ba_linearizer with the graph backend,
    i.e. the code path of `bench.py --gpus N` (the packed Hll | bl | chi2 all-reduce is issued when world_size > 1; with one rank the call
    sequence up to the collective is what runs here, and an explicit all_reduce of the packed buffer checks RCCL accepts it)."""
    import os
    import socket
    import torch
    import torch.distributed as dist
    from openvslam_amd import ba
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        d = synth_local_ba(n_pose=10, n_pt=1500, obs_per_pose=400, seed=13)
        lin = ba.local_ba_linearizer(d["cam"], d["huber_delta"])
        P, F, X = torch.from_numpy(d["poses"]).cuda(), torch.from_numpy(d["pose_fixed"]).cuda(), torch.from_numpy(d["points"]).cuda()
        E = torch.from_numpy(d["edges"].view(np.uint8)).cuda()
        out = lin.linearize(P, F, X, E)
        packed = lin.backend._out["packed"]
        before = packed.clone()
        dist.all_reduce(packed[:12 * 1500 + 2], op=dist.ReduceOp.SUM)     # sum over one rank: unchanged
        torch.cuda.synchronize()
        assert torch.equal(before, packed)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        want = oracle.ba_linearize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], d["huber_delta"])
        assert np.array_equal(got["Hpl"], want["Hpl"]) and np.array_equal(got["Hll"], want["Hll"]) and np.array_equal(got["bl"], want["bl"])
        for k in ("Hpp", "bp", "chi2"):
            assert np.allclose(got[k], want[k], rtol=1e-13, atol=1e-13 * np.abs(want[k]).max()), k
    finally:
        dist.destroy_process_group()


def test_native_multi_device_entry_one_gpu(oracle):
    """ovs_ba_multi_* (the native sharded entry) with n_gpus = 1: same partition / collect code as N devices, no communicator.
    More devices than the box has must fail loudly."""
    import ctypes as C
    from openvslam_amd import _lib, ba
    from oracle import lba
    from test_ba import _lba_scene
    L = _lib.lib()
    d, mono, st, bf, _, _ = _lba_scene(31, n_pose=9, n_pt=1200, obs_per_pose=400, stereo_frac=0.3)
    n_pose, n_pt = len(d["poses"]), len(d["points"])
    cam = ba.BaCam(*d["cam"])
    h = C.c_void_p()
    fixed = np.ascontiguousarray(d["pose_fixed"], np.uint8)
    _lib.check(L.ovs_ba_multi_create(1, n_pose, fixed.ctypes.data, n_pt, mono.ctypes.data, len(mono), st.ctypes.data, len(st), C.byref(cam), bf,
                                     C.byref(h)), "ovs_ba_multi_create")
    try:
        out = dict(Hpp=np.zeros((n_pose, 6, 6)), bp=np.zeros((n_pose, 6)), Hll=np.zeros((n_pt, 3, 3)), bl=np.zeros((n_pt, 3)),
                   Hpl=np.zeros((len(mono) + len(st), 6, 3)), chi2=np.zeros(2))
        P, X = np.ascontiguousarray(d["poses"]), np.ascontiguousarray(d["points"])
        _lib.check(L.ovs_ba_multi_linearize(h, P.ctypes.data, X.ctypes.data, lba.SQRT_CHI2_MONO, lba.SQRT_CHI2_STEREO, out["Hpp"].ctypes.data,
                                            out["bp"].ctypes.data, out["Hll"].ctypes.data, out["bl"].ctypes.data, out["Hpl"].ctypes.data,
                                            out["chi2"].ctypes.data), "ovs_ba_multi_linearize")
    finally:
        L.ovs_ba_multi_destroy(h)
    want = oracle.ba_linearize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], lba.SQRT_CHI2_MONO)
    s = oracle.ba_linearize_stereo(d["poses"], d["pose_fixed"], d["points"], st, d["cam"], bf, lba.SQRT_CHI2_STEREO)
    for k in ("Hpp", "bp", "Hll", "bl", "chi2"):
        want[k] = want[k] + s[k]
    want["Hpl"] = np.concatenate([want["Hpl"], s["Hpl"]])
    assert np.array_equal(out["Hpl"], want["Hpl"]) and np.array_equal(out["Hll"], want["Hll"]) and np.array_equal(out["bl"], want["bl"])
    for k in ("Hpp", "bp", "chi2"):
        assert np.allclose(out[k], want[k], rtol=1e-13, atol=1e-13 * np.abs(want[k]).max()), k
    h2 = C.c_void_p()
    n_dev = L.ovs_device_count()
    if n_dev < 8:
        assert L.ovs_ba_multi_create(n_dev + 1, n_pose, fixed.ctypes.data, n_pt, mono.ctypes.data, len(mono), st.ctypes.data, len(st), C.byref(cam),
                                     bf, C.byref(h2)) == -2


def test_native_multi_device_entry_two_gpus(oracle):
    """ovs_ba_multi_* with n_gpus = 2 (needs two devices on the node: skipped on the 1-GPU test box, run by the driver's multi-GPU tier):
    both exchange variants -- packed RCCL all-reduce and direct xGMI peer sums -- against the one-device result."""
    import json
    import os
    import subprocess
    import sys
    from openvslam_amd import _lib
    if _lib.lib().ovs_device_count() < 2:
        pytest.skip("needs >= 2 HIP devices")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "ba_multi_bench.py"), "2", "12", "3000", "600", "3"], capture_output=True, text=True,
                         timeout=300)
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert "error" not in res, res
    for name in ("rccl", "peer"):
        assert name + "_error" not in res, res
        assert res[name + "_pose_blocks_and_Hpl_bit_equal_to_one_device"] and res[name + "_landmark_sums_max_rel_diff"] < 1e-10, res
    assert res["peer_reproducible"]


# ---- round 4: the reduced camera system on the device (csrc/ba_solve.hip) ----------------------------------------------------------------
def _spd(rng, n, cond):
    """A dense symmetric positive definite matrix with the given condition number (random orthogonal basis, log-spaced spectrum)."""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = np.logspace(0, np.log10(cond), n)
    S = (q * w) @ q.T
    return 0.5 * (S + S.T)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 6, 15, 16, 17, 30, 33, 48, 96, 144, 150, 208, 256, 272, 282, 287, 288, 289, 304, 600, 1024])
def test_dense_solve_matches_numpy(n):
    """The dense solver alone (ovs_ba_dense_solve: k_chol_resident up to 288 unknowns -- trailing tiles in registers / LDS, every tile-row count from 1
    to 18 --, k_chol_solve beyond): blocked Cholesky on the f64 matrix cores + both substitutions against numpy's LAPACK solve,
    at sizes that are / are not multiples of the 16-column panel, up to the largest system the one-workgroup solver stages. The error of a
    backward-stable solve is ~cond * eps relative; twice the same call gives the same bits."""
    from openvslam_amd import ba
    rng = np.random.default_rng(100 + n)
    for cond in (1e2, 1e8):
        S = _spd(rng, n, cond)
        x_true = rng.standard_normal(n)
        rhs = S @ x_true
        x = ba.dense_solve(S, rhs)
        want = np.linalg.solve(S, rhs)
        err = np.abs(x - want).max() / np.abs(want).max()
        assert err < 50 * cond * 2.2e-16 + 1e-13, (n, cond, err)
        assert np.array_equal(x, ba.dense_solve(S, rhs))
    # the lower triangle is what is read: garbage above the diagonal changes nothing
    S2 = S.copy()
    S2[np.triu_indices(n, 1)] = 1e300
    assert np.array_equal(ba.dense_solve(S2, rhs), x)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [48, 288, 304])
def test_dense_solve_failure_then_success(n):
    """launch_dense_solve's contract (ba_solve.hip): a system that is not positive definite is REPORTED (OVS_ERR_INVALID, never a silent NaN solution),
    for the register-resident kernel (n <= 288) and the through-memory one alike, and the next solve of a positive definite system is unaffected."""
    from openvslam_amd import ba
    rng = np.random.default_rng(7 + n)
    S = _spd(rng, n, 1e3)
    rhs = rng.standard_normal(n)
    bad = S.copy()
    bad[n // 2, n // 2] = -abs(bad[n // 2, n // 2])   # a negative pivot in the middle of the factorisation
    with pytest.raises(Exception):
        ba.dense_solve(bad, rhs)
    nan = S.copy()
    nan[0, 0] = np.nan
    with pytest.raises(Exception):
        ba.dense_solve(nan, rhs)
    x = ba.dense_solve(S, rhs)
    want = np.linalg.solve(S, rhs)
    assert np.all(np.isfinite(x)) and np.abs(x - want).max() / np.abs(want).max() < 1e-10


# ---- the dense solver against an extended-precision reference (tests/dense_ref.py) ----------------------------------------------------------
# Criterion: the normwise backward error max|b - S x| / (||S||_inf ||x||_inf + ||b||_inf), evaluated in long double, is at most 10 x the one
# LAPACK's f64 solve reaches on the same system (0.05 .. 0.25 eps on the dense family, test_dense_ref.py). An order of magnitude because the
# kernels multiply by Newton-refined reciprocal square roots (a few ulp each) where LAPACK divides by correctly rounded roots, and sum in the
# matrix cores' 16 x 16 x 4 order: small constant factors. A stale broadcast or a misplaced tile is wrong by more than 1e3 eps, and a tile
# update wrong from its 12th digit on by 95 .. 1660 x LAPACK (test_dense_ref.py), which the forward-error tolerance above lets through.
BERR_MARGIN = 10.0


def _berr_ratio(S, rhs, x, tag):
    """berr(x) / berr(LAPACK's solve of the same system); printed, and appended to the file OVS_BERR_REPORT names."""
    import dense_ref as dr
    lap = dr.backward_error(S, np.linalg.solve(S, rhs), rhs)
    got = dr.backward_error(S, x, rhs)
    ratio = got / lap if lap > 0 else (0.0 if got == 0 else np.inf)
    line = "%-52s device %.4f eps   LAPACK %.4f eps   ratio %.3f" % (tag, got / dr.EPS, lap / dr.EPS, ratio)
    print(line)
    if os.environ.get("OVS_BERR_REPORT"):
        with open(os.environ["OVS_BERR_REPORT"], "a") as f:
            f.write(line + "\n")
    return ratio


def _need_reference(n):
    import dense_ref as dr
    if dr.available(n):
        pytest.skip(dr.available(n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 6, 15, 16, 17, 30, 33, 48, 96, 144, 150, 208, 256, 272, 282, 287, 288, 289, 304, 600, 1024])
def test_dense_solve_backward_error(n):
    """The sizes of test_dense_solve_matches_numpy at cond 1e2, 1e8 and 1e12: the device solve's backward error within 10 x LAPACK's, whatever
    the condition number. The ratio of every case is printed, and appended to the file OVS_BERR_REPORT names. Measured on an MI355X
    (profiles/r07a_dense_solve_backward_error.txt): worst ratio 3.69 of the 63 cases (n = 16, cond 1e2: 0.28 eps against LAPACK's 0.076)."""
    import dense_ref as dr
    from openvslam_amd import ba
    _need_reference(n)
    rng = np.random.default_rng(300 + n)
    for cond in (1e2, 1e8, 1e12):
        S = dr.spd_random_orthogonal(rng, n, cond)
        rhs = S @ rng.standard_normal(n)
        x = ba.dense_solve(S, rhs)
        assert np.all(np.isfinite(x))
        ratio = _berr_ratio(S, rhs, x, "orthogonal n=%d cond=%g" % (n, cond))
        assert ratio <= BERR_MARGIN, (n, cond, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf", [8, 48, 100])
def test_dense_solve_reduced_camera_system(n_kf):
    """What the solver gets in production: J^T J of rows touching two 6-wide keyframe blocks, rotation : translation scales 1 : 300, 1e-4 of the
    diagonal as damping, most off-diagonal 6 x 6 blocks exactly zero; 48, 288 (k_chol_resident) and 600 unknowns (k_chol_solve). Same
    criterion. Measured: worst ratio 2.85 (48 keyframes, random rhs: 0.0013 eps against 0.0005)."""
    import dense_ref as dr
    from openvslam_amd import ba
    _need_reference(6 * n_kf)
    rng = np.random.default_rng(n_kf)
    S, pairs = dr.ba_reduced_system(rng, n_kf)
    assert dr.zero_blocks(S) == n_kf * (n_kf - 1) // 2 - len(pairs) > 0        # exact-zero off-diagonal blocks are there
    for tag, rhs in (("random rhs", rng.standard_normal(6 * n_kf)), ("rhs = S x", S @ rng.standard_normal(6 * n_kf))):
        x = ba.dense_solve(S, rhs)
        ratio = _berr_ratio(S, rhs, x, "reduced camera system %d keyframes, %s" % (n_kf, tag))
        assert ratio <= BERR_MARGIN, (n_kf, tag, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [96, 288, 304])
def test_dense_solve_block_diagonal(n):
    """Block-diagonal systems whose block boundaries are off the 16-column panel grid (6 + 30 + 17 + ...): the whole system meets the
    criterion, and so does EVERY block of the whole system's solution against that block's own system (a leak between blocks hides behind the
    norm of the largest one otherwise), as does the block solved alone. Measured: worst ratio 1.85 (n = 304, the 17-row block of the whole system's solution)."""
    import dense_ref as dr
    from openvslam_amd import ba
    _need_reference(n)
    rng = np.random.default_rng(n)
    S, blocks = dr.block_diagonal(rng, dr.BLOCK_SIZES[n])
    rhs = rng.standard_normal(n)
    x = ba.dense_solve(S, rhs)
    assert _berr_ratio(S, rhs, x, "block diagonal n=%d, whole" % n) <= BERR_MARGIN
    for i, b in enumerate(blocks):
        Sb, rb = np.ascontiguousarray(S[b, b]), rhs[b]
        r_whole = _berr_ratio(Sb, rb, x[b], "block diagonal n=%d, block %d (%d) of the whole" % (n, i, b.stop - b.start))
        r_alone = _berr_ratio(Sb, rb, ba.dense_solve(Sb, rb), "block diagonal n=%d, block %d (%d) alone" % (n, i, b.stop - b.start))
        assert r_whole <= BERR_MARGIN and r_alone <= BERR_MARGIN, (n, i, r_whole, r_alone)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 48, 288, 304, 600])
def test_dense_solve_zero_rhs_gives_zero(n):
    import dense_ref as dr
    from openvslam_amd import ba
    S = dr.spd_random_orthogonal(np.random.default_rng(n), n, 1e6)
    assert np.array_equal(ba.dense_solve(S, np.zeros(n)), np.zeros(n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 48, 288, 304, 600])
def test_dense_solve_refuses_at_every_pivot_class(n):
    """S = L L^T from an integer L with powers of two on its diagonal: the factorisation is exact in f64, so subtracting L[k][k]^2 from
    S[k][k] makes pivot k EXACTLY zero and subtracting twice that makes it negative. Every lane class of the 16-row block (first, 14, 15 -- the
    last of a block --, 16, 31), the first rows of the last 17 and the last two pivots: each is refused (OVS_ERR_INVALID; never a returned
    NaN), as are +inf on a diagonal entry of the last block and a NaN in the last row, and after each refusal the unmodified system is solved
    within the criterion (measured: worst ratio 4.01, n = 288). (Invalid data on the documented error path, once each.)"""
    import dense_ref as dr
    from openvslam_amd import ba
    _need_reference(n)
    rng = np.random.default_rng(n)
    S, L = dr.integer_factor_system(rng, n)
    rhs = rng.standard_normal(n)

    def still_solves(tag):
        x = ba.dense_solve(S, rhs)
        assert np.all(np.isfinite(x))
        assert _berr_ratio(S, rhs, x, "integer factor n=%d after %s" % (n, tag)) <= BERR_MARGIN, (n, tag)

    still_solves("nothing")
    for k in dr.pivot_classes(n):
        for what, times in (("zero", 1.0), ("negative", 2.0)):
            bad = S.copy()
            bad[k, k] -= times * L[k, k] ** 2
            with pytest.raises(RuntimeError, match="positive definite"):
                ba.dense_solve(bad, rhs)
            still_solves("%s pivot %d" % (what, k))
    inf = S.copy()
    inf[n - 2, n - 2] = np.inf
    with pytest.raises(RuntimeError):
        ba.dense_solve(inf, rhs)
    still_solves("+inf at the diagonal of row %d" % (n - 2))
    nan = S.copy()
    nan[n - 1, n // 3] = np.nan
    with pytest.raises(RuntimeError):
        ba.dense_solve(nan, rhs)
    still_solves("NaN in the last row")


@pytest.mark.gpu
def test_local_ba_alternative_paths_give_the_same_bits_and_match_the_oracle(tmp_path, oracle):
    """Two process-wide switches (read once per process, so each runs in a child) select paths of ovs_local_ba_optimize that production
    does not take at this size: a trial's outcome through a D2H copy and a stream wait instead of the flag-carrying words the host polls
    (OVS_BA_LL_NOTIFY=0), and the pairs' common landmarks found by every trial's k_schur itself instead of once per graph by k_pair_lists
    (OVS_BA_SCHUR_LISTS=0; production above the pair-list bound). Both must give the default's bits on one linearisation and on a whole
    ovs_local_ba_optimize, stereo edges included (stereo 0.35, 3000 landmarks). The default is checked against the oracle on the same scene:
    the linearisation at the tolerances of test_graph_linearize_is_deterministic_and_matches_oracle, the optimisation at those of
    test_local_ba_optimize."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
from oracle import lba
from openvslam_amd import ba
from test_ba import _lba_scene
d, mono, st, bf, _, _ = _lba_scene(21, n_pose=12, n_pt=3000, obs_per_pose=700, stereo_frac=0.35)
g = ba.graph(len(d["poses"]), d["pose_fixed"], len(d["points"]), mono, d["cam"], st, bf)
out = g.linearize_dev(torch.from_numpy(d["poses"]).cuda(), torch.from_numpy(d["points"]).cuda(), lba.SQRT_CHI2_MONO, lba.SQRT_CHI2_STEREO)
torch.cuda.synchronize()
res = {"lin_" + k: t.cpu().numpy() for k, t in ba.graph.views(out, g.n_pose, g.n_pt, g.n_edge).items()}
r = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], st, bf)
res.update({"opt_" + k: np.asarray(v) for k, v in r.items()})
np.savez(sys.argv[1], **res)
"""
    outs = {}
    variants = (("auto", {}), ("copies", {"OVS_BA_LL_NOTIFY": "0"}), ("schur_scan", {"OVS_BA_SCHUR_LISTS": "0"}))
    for tag, env in variants:
        out = tmp_path / ("%s.npz" % tag)
        r = subprocess.run([sys.executable, "-c", code % (root, os.path.join(root, "tests")), str(out)], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = dict(np.load(out))
    got = outs["auto"]
    assert len(got) >= 10 and got["opt_info"][4] >= 3
    for tag, _ in variants[1:]:
        for k, v in got.items():
            assert np.array_equal(v, outs[tag][k]), (tag, k)
    # the default against the oracle on the same scene
    from oracle import lba
    from test_ba import _lba_scene
    d, mono, st, bf, _, _ = _lba_scene(21, n_pose=12, n_pt=3000, obs_per_pose=700, stereo_frac=0.35)
    hm, hs = lba.SQRT_CHI2_MONO, lba.SQRT_CHI2_STEREO
    want = oracle.ba_linearize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], hm)
    s = oracle.ba_linearize_stereo(d["poses"], d["pose_fixed"], d["points"], st, d["cam"], bf, hs)
    for k in ("Hpp", "bp", "Hll", "bl", "chi2"):
        want[k] = want[k] + s[k]
    want["Hpl"] = np.concatenate([want["Hpl"], s["Hpl"]])
    for k in ("Hpl", "Hll", "bl"):
        assert np.array_equal(got["lin_" + k], want[k]), k
    for k in ("Hpp", "bp", "chi2"):
        scale = np.abs(want[k]).max()
        assert np.allclose(got["lin_" + k], want[k], rtol=1e-13, atol=1e-13 * scale), k
    free = d["pose_fixed"] == 0
    md = max(np.abs(np.einsum("kii->ki", want["Hpp"][free])).max(), np.abs(np.einsum("kii->ki", want["Hll"])).max())
    assert np.isclose(got["lin_max_diag"][0], md, rtol=1e-13)
    want = lba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], st, bf)
    assert np.array_equal(got["opt_info"][4:], want["info"][4:]) and want["info"][4] >= 3
    assert np.allclose(got["opt_info"][:4], want["info"][:4], rtol=1e-7)
    assert np.allclose(got["opt_poses"], want["poses"], rtol=1e-7, atol=1e-8)
    assert np.allclose(got["opt_points"], want["points"], rtol=1e-7, atol=1e-8)
    for k in ("mono_outlier", "stereo_outlier"):
        assert (got["opt_" + k] != want[k]).sum() <= max(1, len(want[k]) // 5000), k
    fixed = d["pose_fixed"].astype(bool)
    assert np.array_equal(got["opt_poses"][fixed], d["poses"][fixed])


@pytest.mark.gpu
def test_a_landmark_with_more_edges_than_a_workgroup_has_lanes(tmp_path, oracle):
    """A landmark seen by 270 keyframes (168 free: the device solver's size) is a workgroup of its own in k_linearize2's landmark partition and
    in k_trial_update's one-lane-per-edge back-substitution, its edges passing in pieces of 256. The whole optimisation against the oracle, and
    bit-equal to the one with every trial's k_schur scanning for the pairs' common landmarks (OVS_BA_SCHUR_LISTS=0, a child process)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from openvslam_amd import ba
from openvslam_amd.synth import synth_local_ba
from openvslam_amd.ba import EDGE_DTYPE, quat_to_rot
d = synth_local_ba(n_pose=270, n_pt=400, obs_per_pose=60, seed=5, pose_noise=0.01, point_noise=0.01, n_fixed=102)
e = d["edges"]
rng = np.random.default_rng(9)
extra = []
for j in (0, 7):   # two landmarks observed by EVERY keyframe
    have = set(e["pose_idx"][e["point_idx"] == j].tolist())
    for k in range(270):
        if k in have: continue
        pc = quat_to_rot(d["poses_true"][k, 3:]) @ d["points_true"][j] + d["poses_true"][k, :3]
        r = np.zeros(1, EDGE_DTYPE)
        r["pose_idx"], r["point_idx"] = k, j
        r["obs_x"] = d["cam"][0] * pc[0] / pc[2] + d["cam"][2] + rng.normal()
        r["obs_y"] = d["cam"][1] * pc[1] / pc[2] + d["cam"][3] + rng.normal()
        r["inv_sigma_sq"] = 1.0
        extra.append(r)
edges = np.concatenate([e] + extra)
edges = edges[rng.permutation(len(edges))]
assert (edges["point_idx"] == 0).sum() == 270
r = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], edges, d["cam"])
np.savez(sys.argv[1], edges=edges, **{"opt_" + k: np.asarray(v) for k, v in r.items()})
"""
    outs = {}
    variants = (("auto", {}), ("schur_scan", {"OVS_BA_SCHUR_LISTS": "0"}))
    for tag, env in variants:
        out = tmp_path / ("%s.npz" % tag)
        r = subprocess.run([sys.executable, "-c", code % (root, os.path.join(root, "tests")), str(out)], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = dict(np.load(out))
    info = outs["auto"]["opt_info"]
    assert info[4] >= 3 and info[3] < info[0]
    for tag, _ in variants[1:]:
        for k, v in outs["auto"].items():
            assert np.array_equal(v, outs[tag][k]), (tag, k)
    # and the device against the oracle (the test_local_ba_optimize tolerance)
    from oracle import lba
    d = synth_local_ba(n_pose=270, n_pt=400, obs_per_pose=60, seed=5, pose_noise=0.01, point_noise=0.01, n_fixed=102)
    want = lba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], outs["auto"]["edges"], d["cam"])
    assert np.array_equal(info[4:], want["info"][4:])
    assert np.allclose(outs["auto"]["opt_poses"], want["poses"], rtol=1e-7, atol=1e-8)
    assert np.allclose(outs["auto"]["opt_points"], want["points"], rtol=1e-7, atol=1e-8)
    assert (outs["auto"]["opt_mono_outlier"] != want["mono_outlier"]).sum() <= 1


@pytest.mark.gpu
def test_resident_and_through_memory_solvers_agree(tmp_path):
    """k_chol_resident (default up to 288 unknowns) against k_chol_solve (OVS_CHOL_RESIDENT=0, a process-wide switch: run in a child process) on the
    same systems: the two differ in the order of the fused multiply-adds only (~cond x 1e-16 relative); the phase-timed instantiation
    (OVS_BA_TRACE) returns the product instantiation's bits."""
    import subprocess
    import sys
    from openvslam_amd import ba
    rng = np.random.default_rng(77)
    cases = {}
    for n in (40, 96, 200, 288):
        S = _spd(rng, n, 1e4)
        rhs = rng.standard_normal(n)
        cases["S%d" % n], cases["r%d" % n] = S, rhs
    np.savez(tmp_path / "in.npz", **cases)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); from openvslam_amd import ba; d = np.load(%r); "
            "np.savez(%r, **{'x%%s' %% k[1:]: ba.dense_solve(d[k], d['r' + k[1:]]) for k in d.files if k[0] == 'S'})")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for tag, env in (("mem", {"OVS_CHOL_RESIDENT": "0"}), ("timed", {"OVS_BA_TRACE": "1"})):
        out = tmp_path / ("out_%s.npz" % tag)
        r = subprocess.run([sys.executable, "-c", code % (root, str(tmp_path / "in.npz"), str(out))], env=dict(os.environ, **env), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.load(out)
        for n in (40, 96, 200, 288):
            x = ba.dense_solve(cases["S%d" % n], cases["r%d" % n])
            if tag == "timed":
                assert np.array_equal(got["x%d" % n], x), n
                assert "dense solve n=%d" % n in r.stderr
            else:
                assert np.abs(got["x%d" % n] - x).max() <= 1e-10 * np.abs(x).max(), n


@pytest.mark.gpu
def test_dense_solve_reports_a_matrix_that_is_not_positive_definite():
    from openvslam_amd import ba
    rng = np.random.default_rng(7)
    for n, bad_at in ((48, 5), (48, 40), (50, 49), (288, 3), (288, 280), (400, 17)):
        S = _spd(rng, n, 10.0)
        S[bad_at, bad_at] = -1.0   # an indefinite matrix: some pivot at or before `bad_at` is not positive
        with pytest.raises(RuntimeError, match="positive definite"):
            ba.dense_solve(S, np.ones(n))
    with pytest.raises(RuntimeError):
        ba.dense_solve(np.eye(1025), np.ones(1025))   # beyond the solver's LDS


@pytest.mark.gpu
@pytest.mark.parametrize("stereo_frac,n_pose,n_pt,obs", [(0.3, 10, 1500, 500), (0.0, 50, 20000, 2000)])
def test_local_ba_device_and_host_solver_agree(stereo_frac, n_pose, n_pt, obs):
    """ovs_local_ba_optimize with the reduced camera system solved on the device (default) and on the host (rounds 1-3): the same
    Levenberg-Marquardt path -- iteration counts, accepted / rejected trials -- and states equal to 1e-9 (the two solves differ in
    operation order only; the oracle comparison of test_local_ba_optimize runs on the default)."""
    from openvslam_amd import ba
    from test_ba import _lba_scene
    d, mono, st, bf, _, _ = _lba_scene(3, n_pose=n_pose, n_pt=n_pt, obs_per_pose=obs, stereo_frac=stereo_frac)
    assert ba.local_ba_get_solver() == "device"
    dev = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], st, bf)
    try:
        ba.local_ba_set_solver("host")
        host = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], st, bf)
    finally:
        ba.local_ba_set_solver("device")
    assert np.array_equal(dev["info"][4:], host["info"][4:])
    assert np.allclose(dev["info"][:4], host["info"][:4], rtol=1e-9)
    assert np.allclose(dev["poses"], host["poses"], rtol=1e-9, atol=1e-10), np.abs(dev["poses"] - host["poses"]).max()
    assert np.allclose(dev["points"], host["points"], rtol=1e-9, atol=1e-10)
    for k in ("mono_outlier", "stereo_outlier"):
        assert np.array_equal(dev[k], host[k]), k
    again = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], st, bf)
    assert np.array_equal(again["poses"], dev["poses"]) and np.array_equal(again["points"], dev["points"])   # no atomics anywhere


@pytest.mark.gpu
def test_local_ba_with_every_keyframe_fixed_and_with_one_free(oracle):
    """The reduced camera system's edge sizes: no free keyframe (only landmarks move: no system to solve) and a single free keyframe (6
    unknowns inside one padded 16 x 16 block), both against the oracle."""
    from oracle import lba
    from openvslam_amd import ba
    from test_ba import _lba_scene
    d, mono, st, bf, _, _ = _lba_scene(5, n_pose=6, n_pt=600, obs_per_pose=300, stereo_frac=0.2)
    for n_free in (0, 1):
        fixed = np.ones(len(d["poses"]), np.uint8)
        fixed[len(fixed) - n_free:] = 0
        got = ba.local_ba_optimize(d["poses"], fixed, d["points"], mono, d["cam"], st, bf)
        want = lba.local_ba_optimize(d["poses"], fixed, d["points"], mono, d["cam"], st, bf)
        # with landmarks only the second round converges inside its 10 iterations, and the iteration it stops at is decided by the sign of a
        # gain ratio that is rounding noise by then (ORACLE_SPEC rule 25): 8 here, 9 in the oracle, at chi2 equal to every printed digit.
        # Iteration counts may therefore differ by one where the cost agrees to 1e-9.
        assert got["info"][4] == want["info"][4] and abs(got["info"][5] - want["info"][5]) <= 1
        assert np.allclose(got["info"][:4], want["info"][:4], rtol=1e-9)
        assert np.allclose(got["points"], want["points"], rtol=1e-7, atol=1e-8)
        assert np.allclose(got["poses"], want["poses"], rtol=1e-7, atol=1e-8)
        assert np.array_equal(got["poses"][fixed.astype(bool)], d["poses"][fixed.astype(bool)])


@pytest.mark.gpu
def test_local_ba_beyond_the_device_solvers_size_takes_the_host_solve():
    """More than 1024 unknowns (172 free keyframes): ovs_local_ba_optimize solves the reduced camera system on the host as in rounds 1-3; the
    result must not depend on the solver setting then, and the optimisation must still converge."""
    from openvslam_amd import ba
    d = synth_local_ba(n_pose=174, n_pt=6000, obs_per_pose=400, seed=3, pose_noise=0.02, point_noise=0.02, n_fixed=2)
    a = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"])
    try:
        ba.local_ba_set_solver("host")
        b = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"])
    finally:
        ba.local_ba_set_solver("device")
    assert np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["points"], b["points"])
    assert a["info"][3] < 0.5 * a["info"][0] and a["info"][4] >= 3


@pytest.mark.gpu
def test_local_ba_edge_counts_order_and_threads():
    """The late-round-6 data paths at their corners: no edge at all, one edge, 63 / 65 edges (a wave's staged records and their fall-back), an edge
    list that is NOT keyframe-major (every lane stores its own Hpl record), and two threads calling at once (page-locked images and blocks are per
    thread): finite states, the same flags, and the same bits from both threads as from a single-threaded call."""
    import threading
    from openvslam_amd import ba
    d = synth_local_ba(n_pose=6, n_pt=300, obs_per_pose=100, seed=1, pose_noise=0.01, point_noise=0.01, n_fixed=2)
    e = d["edges"]
    for n in (0, 1, 63, 65):
        r = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], e[:n], d["cam"])
        assert np.isfinite(r["poses"]).all() and np.isfinite(r["points"]).all() and len(r["mono_outlier"]) == n
        assert (r["info"][4] == 0) == (n == 0) and r["info"][3] <= r["info"][0]
    r1 = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], e, d["cam"])
    r2 = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], e[::-1].copy(), d["cam"])
    assert np.abs(r1["poses"] - r2["poses"]).max() < 1e-11 and np.abs(r1["points"] - r2["points"]).max() < 1e-11
    assert np.array_equal(r1["mono_outlier"], r2["mono_outlier"][::-1])
    outs = [None, None]

    def work(i):
        for _ in range(10):
            outs[i] = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], e, d["cam"])
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for o in outs:
        assert np.array_equal(o["poses"], r1["poses"]) and np.array_equal(o["points"], r1["points"]) and np.array_equal(o["mono_outlier"], r1["mono_outlier"])
