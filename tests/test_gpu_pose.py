"""GPU parity of optimize::pose_optimizer::optimize (one-launch device Levenberg-Marquardt) against the CPU oracle.
Stated tolerance: pose entries within 1e-9 (the normal-equation sums are associated differently: block tree vs sequential);
inlier / outlier flags identical except observations whose chi2 sits within 1e-6 (relative) of the 5.991 / 7.815 gates.
Equirectangular frames: 2e-8. The LM loop ends a round on the sign of a gain ratio that is rounding noise once the round has
converged, so which trial is the last depends on the summation order; the CPU oracle itself moves by up to 5.2e-9 on these very
frames when its observations are permuted (tests/test_ba.py::test_pose_oracle_order_sensitivity), and so does the device result
between its 256- and 512-thread workgroups."""
import os

import numpy as np
import pytest

import pose_scenes as ps

pytestmark = pytest.mark.gpu


from openvslam_amd.synth import synth_pose_frame as make_frame


@pytest.mark.parametrize("n,stereo_frac,outlier_frac,pose_err", [(1500, 0.4, 0.1, 1.0), (2000, 0.0, 0.2, 2.0), (300, 1.0, 0.05, 0.5), (7, 0.5, 0.0, 1.0),
                                                                 (3, 0.0, 0.0, 1.0), (8192, 0.3, 0.15, 1.0)])
def test_pose_optimize(oracle, n, stereo_frac, outlier_frac, pose_err):
    from openvslam_amd import ba
    T0, obs, cam, bf, (Rt, tt, bad) = make_frame(oracle.POSE_OBS_DTYPE, n, n, stereo_frac, outlier_frac, pose_err)
    T, out, nv = ba.pose_optimize(T0, obs, cam, bf)
    wT, wout, wnv = oracle.pose_optimize(T0, obs, cam, bf)
    assert np.allclose(T, wT, rtol=0, atol=1e-9)
    diff = np.nonzero(out != wout)[0]
    if len(diff):   # only observations sitting on a chi2 gate may flip
        pc = obs["pos_w"][diff] @ wT[:, :3].T + wT[:, 3]
        u = cam[0] * pc[:, 0] / pc[:, 2] + cam[2]
        e2 = (obs["obs_x"][diff] - u) ** 2 + (obs["obs_y"][diff] - (cam[1] * pc[:, 1] / pc[:, 2] + cam[3])) ** 2
        e2 += np.where(obs["is_stereo"][diff] != 0, (obs["obs_x_right"][diff] - (u - bf / pc[:, 2])) ** 2, 0)
        c2 = e2 * obs["inv_sigma_sq"][diff]
        gate = np.where(obs["is_stereo"][diff] != 0, 7.815, 5.991)
        assert np.all(np.abs(c2 - gate) < 1e-6 * gate)
    assert abs(nv - wnv) <= len(diff)
    if n >= 300:
        assert np.linalg.norm(wT[:, 3] - tt) < 0.02 and (wout == bad).mean() > 0.9
    if n < 5:
        assert nv == 0 and np.array_equal(T, T0)


@pytest.mark.parametrize("n,stereo_frac,outlier_frac,pose_err", [(1500, 0.4, 0.1, 1.0), (2000, 0.0, 0.25, 3.0)])
def test_pose_optimize_reset_each_round_variant(oracle, n, stereo_frac, outlier_frac, pose_err):
    """ORACLE_SPEC rule 25 (iv) as a run-time variant of BOTH sides (ovs_pose_set_variant / ovo_pose_set_variant): ORB-SLAM2's re-set of the
    frame vertex at the start of every round. Same tolerance as the default schedule; and the variant is not a no-op."""
    from openvslam_amd import ba
    T0, obs, cam, bf, _ = make_frame(oracle.POSE_OBS_DTYPE, n, n, stereo_frac, outlier_frac, pose_err)
    T_def, out_def, _ = ba.pose_optimize(T0, obs, cam, bf)
    try:
        ba.pose_set_variant("reset_each_round", 1)
        oracle.pose_set_variant("reset_each_round", 1)
        T, out, nv = ba.pose_optimize(T0, obs, cam, bf)
        wT, wout, wnv = oracle.pose_optimize(T0, obs, cam, bf)
    finally:
        ba.pose_set_variant("reset_each_round", 0)
        oracle.pose_set_variant("reset_each_round", 0)
    assert np.allclose(T, wT, rtol=0, atol=1e-9) and (out != wout).sum() <= 2 and abs(nv - wnv) <= 2
    assert not np.array_equal(T, T_def)   # another schedule: the last bits of the pose differ
    assert np.allclose(T, T_def, rtol=0, atol=1e-4)   # ... and only those: both converge to the same optimum
    T2, _, _ = ba.pose_optimize(T0, obs, cam, bf)
    assert np.array_equal(T2, T_def)      # the default is back


# ---- equirectangular frames (BASELINE configs[3]: 3840 x 1920): equirectangular_pose_opt_edge
@pytest.mark.parametrize("n,outlier_frac,pose_err,seam,pole", [(1500, 0.1, 1.0, 0.0, 0.0), (2000, 0.2, 2.0, 0.1, 0.05), (300, 0.05, 0.5, 0.3, 0.3),
                                                               (7, 0.0, 1.0, 0.0, 0.0), (3, 0.0, 1.0, 0.0, 0.0), (8192, 0.15, 1.0, 0.05, 0.05)])
def test_pose_optimize_equirect(oracle, n, outlier_frac, pose_err, seam, pole):
    from openvslam_amd import ba
    from openvslam_amd.synth import equirect_project, synth_pose_frame_equirect
    T0, obs, cols, rows, (Rt, tt, bad) = synth_pose_frame_equirect(oracle.POSE_OBS_DTYPE, n, 100 + n, outlier_frac=outlier_frac, pose_err=pose_err,
                                                                   seam_frac=seam, pole_frac=pole)
    T, out, nv = ba.pose_optimize_equirect(T0, obs, cols, rows)
    wT, wout, wnv = oracle.pose_optimize_equirect(T0, obs, cols, rows)
    assert np.allclose(T, wT, rtol=0, atol=2e-8)
    diff = np.nonzero(out != wout)[0]
    if len(diff):   # only observations sitting on the chi2 gate may flip
        u, v = equirect_project(obs["pos_w"][diff] @ wT[:, :3].T + wT[:, 3], cols, rows)
        c2 = ((obs["obs_x"][diff] - u) ** 2 + (obs["obs_y"][diff] - v) ** 2) * obs["inv_sigma_sq"][diff]
        assert np.all(np.abs(c2 - 5.991) < 1e-6 * 5.991)
    assert abs(nv - wnv) <= len(diff)
    if n >= 300 and seam == 0.0:
        assert np.linalg.norm(wT[:, 3] - tt) < 0.05 and (wout == bad).mean() > 0.9
    if n < 5:
        assert nv == 0 and np.array_equal(T, T0)


def test_single_frame_groups_agree_with_the_batch_form():
    """Round 4: ovs_pose_optimize spreads one frame with >= 1200 observations over four workgroups (grid barrier per pass, partial sums added
    in workgroup order); ovs_pose_optimize_batch_dev runs one workgroup per frame. Same schedule, sums associated differently: poses to 2e-8
    (ORACLE_SPEC rule 25: which trial a converged round ends on is rounding noise; 2.1e-9 seen), the same inlier flags (no observation of
    these frames sits on a chi2 gate), and each form gives the same bits twice."""
    import ctypes as C
    import torch
    from openvslam_amd import _lib, ba
    from oracle import binding as ob
    L = _lib.lib()
    frames = [make_frame(ob.POSE_OBS_DTYPE, n, seed, stereo_frac=sf, outlier_frac=0.1) for n, seed, sf in ((1800, 3, 0.0), (900, 4, 0.5), (2600, 5, 0.2))]
    cam = frames[0][2]
    bf = frames[0][3]
    obs = np.concatenate([f[1] for f in frames])
    offs = np.cumsum([0] + [len(f[1]) for f in frames]).astype(np.int32)
    T_in = np.stack([np.concatenate([f[0][:, :3].ravel(), f[0][:, 3]]) for f in frames])   # R row-major | t
    d_T = torch.from_numpy(T_in).cuda()
    d_obs = torch.from_numpy(obs.view(np.uint8)).cuda()
    d_off = torch.from_numpy(offs).cuda()
    d_out = torch.empty_like(d_T)
    d_fl = torch.empty(len(obs), dtype=torch.uint8, device="cuda")
    d_nv = torch.empty(len(frames), dtype=torch.int32, device="cuda")
    cam_c = ba.BaCam(*cam)
    torch.cuda.synchronize()
    st = L.ovs_pose_optimize_batch_dev(d_T.data_ptr(), d_obs.data_ptr(), d_off.data_ptr(), len(frames), C.byref(cam_c), float(bf), 1,
                                       d_out.data_ptr(), d_fl.data_ptr(), d_nv.data_ptr(), None)
    assert st == 0
    torch.cuda.synchronize()
    out, fl, nv = d_out.cpu().numpy(), d_fl.cpu().numpy(), d_nv.cpu().numpy()
    for k, (T0, o, _, _, _) in enumerate(frames):
        T1, flags1, nv1 = ba.pose_optimize(T0, o, cam, bf, setup_type=1)
        T1b, flags1b, _ = ba.pose_optimize(T0, o, cam, bf, setup_type=1)
        assert np.array_equal(T1, T1b) and np.array_equal(flags1, flags1b)
        got = np.concatenate([T1[:, :3].ravel(), T1[:, 3]])
        assert np.allclose(got, out[k], rtol=0, atol=2e-8), np.abs(got - out[k]).max()
        assert nv1 == nv[k] and np.array_equal(flags1.astype(np.uint8), fl[offs[k]:offs[k + 1]])


def test_grouped_pose_optimiser_beside_a_saturated_device():
    """The four workgroups of a frame meet at a grid-wide barrier, so they must all become resident while other streams fill the device: 150
    pose optimisations of a 2000-observation frame (four workgroups) beside a thread that keeps 64-frame batch extractions in flight give
    the bits of an undisturbed call every time, and finish (the barrier has a 50 ms bail-out to the one-workgroup form)."""
    import threading
    import torch
    from openvslam_amd import ba, feature
    from openvslam_amd.synth import synth_video
    from oracle import binding as ob
    T0, obs, cam, bf, _ = make_frame(ob.POSE_OBS_DTYPE, 2000, 21)
    ref = ba.pose_optimize(T0, obs, cam, bf)
    rows, cols, B = 480, 752, 64
    ex = feature.orb_extractor(feature.orb_params(1000), max_rows=rows, max_cols=cols, max_batch=B)
    d_img = torch.from_numpy(synth_video(rows, cols, B, seed=5)).cuda()
    cap = ex.max_keypoints
    d_kps = torch.empty((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.empty((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.empty(B, dtype=torch.int32, device="cuda")
    stop = threading.Event()
    busy_stream = torch.cuda.Stream()

    def load():
        while not stop.is_set():
            for _ in range(4):
                ex.extract_batch_dev(d_img, d_kps, d_desc, d_cnt, stream=busy_stream.cuda_stream)
            busy_stream.synchronize()

    th = threading.Thread(target=load)
    th.start()
    try:
        for _ in range(150):
            T, out, nv = ba.pose_optimize(T0, obs, cam, bf)
            assert nv == ref[2] and np.array_equal(T, ref[0]) and np.array_equal(out, ref[1])
    finally:
        stop.set()
        th.join()


def test_batched_retries_give_the_sequential_results(tmp_path):
    """Round 4: after an iteration's first trial is rejected the nine retries g2o would make one by one are solved on nine lanes and
    evaluated in one pass over the observations. Same arithmetic per trial, same decisions in the same order: the results must be the bits
    of the sequential form (OVS_POSE_BATCH_RETRIES=0, read once per process: a child process computes them), for one and for four
    workgroups per frame, perspective and equirectangular."""
    import subprocess
    import sys
    from openvslam_amd import ba
    from openvslam_amd.synth import synth_pose_frame_equirect
    from oracle import binding as ob
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from openvslam_amd import ba\n"
        "from openvslam_amd.synth import synth_pose_frame, synth_pose_frame_equirect\n"
        "from oracle import binding as ob\n"
        "out = {}\n"
        "for n, seed in ((300, 1), (1000, 2), (1300, 3), (2500, 4), (60, 5)):\n"
        "    T0, obs, cam, bf, _ = synth_pose_frame(ob.POSE_OBS_DTYPE, n, seed)\n"
        "    T, fl, nv = ba.pose_optimize(T0, obs, cam, bf)\n"
        "    out['p%%d' %% n] = np.concatenate([T.ravel(), fl.astype(float), [nv]])\n"
        "for n, seed in ((400, 6), (2000, 7)):\n"
        "    T0, obs, cols, rows, _ = synth_pose_frame_equirect(ob.POSE_OBS_DTYPE, n, seed, seam_frac=0.1, pole_frac=0.05)\n"
        "    T, fl, nv = ba.pose_optimize_equirect(T0, obs, cols, rows)\n"
        "    out['e%%d' %% n] = np.concatenate([T.ravel(), fl.astype(float), [nv]])\n"
        "np.savez(sys.argv[1], **out)\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = {}
    # round 6: the same for the forms of the data path -- observations held in registers and read straight from the pinned host block
    # (default), re-read from device memory per pass (OVS_POSE_OBS_REGS=0), registers but through the H2D / D2H copies (OVS_POSE_ZERO_COPY=0)
    variants = (("batched", {}), ("sequential", {"OVS_POSE_BATCH_RETRIES": "0"}), ("from_memory", {"OVS_POSE_OBS_REGS": "0"}),
                ("copies", {"OVS_POSE_ZERO_COPY": "0"}))
    for tag, env in variants:
        f = str(tmp_path / (tag + ".npz"))
        subprocess.check_call([sys.executable, "-c", code, f], env=dict(os.environ, **env), timeout=300)
        res[tag] = np.load(f)
    for tag, _ in variants[1:]:
        assert sorted(res["batched"].files) == sorted(res[tag].files) and len(res["batched"].files) == 7
        for k in res["batched"].files:
            assert np.array_equal(res["batched"][k], res[tag][k]), (tag, k)


# ---- every launch form, size edge and LM exit (tests/pose_scenes.py; the CPU side of these frames: tests/test_pose_scenes.py) -------------------
# The frames are chosen on the CPU so that the oracle's own spread under permutations of the observations is at most a quarter of the tolerance
# and no observation sits on a chi-square gate: pose to 1e-9 (perspective) / 2e-8 (equirectangular), flags and count identical, no exceptions.
_EDGE = tuple(r.name for r in ps.edge_frames())
_EXTRA = tuple(r.name for r in ps.extra_frames())
_SCENES = tuple(s.name for s in ps.scenes())
_GROUP_SCENES = ("zero_weights_p", "perfect_p600", "few_inliers_p5", "survivors_p4", "survivors_p5", "survivors_e4", "behind_camera")


def _group_frames(g):
    """Forced workgroup counts: frames shorter than a workgroup (workgroups that own nothing still publish their 28 zeros at every exchange),
    the two sizes around 2 * g * 256 (registers -> memory) and the largest frame."""
    around = ("p%d" % (2 * g * 256), "p%d" % (2 * g * 256 + 1)) + (("e4096", "e4097") if g == 8 else ())
    return ("p5", "p6", "p255", "p257", "p300") + around + ("p8192", "e5", "e257", "e300", "e8192") + _GROUP_SCENES


# tag -> (environment of the child process, its frames). The switches are read once per process, hence children.
_FORMS = {
    "one_group_256": ({"OVS_POSE_GROUPS": "1", "OVS_POSE_THREADS": "256"}, _EDGE + _EXTRA + _SCENES),   # <MODEL, 256, 2> to 512 observations, <MODEL, 256, 0> above
    "one_group_512": ({"OVS_POSE_GROUPS": "1"}, ("p767", "p768", "p1024", "p2048", "p8192", "e1499", "e1500", "e4097")),   # <MODEL, 512, 0> from 768 / 1500
    "groups2": ({"OVS_POSE_GROUPS": "2"}, _group_frames(2)),
    "groups4": ({"OVS_POSE_GROUPS": "4"}, _group_frames(4)),
    "groups8": ({"OVS_POSE_GROUPS": "8"}, _group_frames(8)),
    "from_memory": ({"OVS_POSE_OBS_REGS": "0"}, _EDGE + _SCENES),   # <MODEL, 256, 0> at the default workgroup counts, through the copies
}
_FORM_CASES = [(tag, name) for tag, (_, names) in _FORMS.items() for name in names]
_CHILD = (
    "import sys\n"
    "sys.path[:0] = [%r, %r]\n"
    "import numpy as np\n"
    "import pose_scenes as ps\n"
    "from openvslam_amd import ba\n"
    "np.savez(sys.argv[1], **{name: ps.pack(*ps.run(ba, ps.frame_by_name(name))) for name in sys.argv[2:]})\n"
    % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(scope="module")
def forced_forms(tmp_path_factory):
    """One child process per forced launch form, one after another, each under its own time limit; a child that fails ends the fixture (no
    further child is started)."""
    import subprocess
    import sys
    base = {k: v for k, v in os.environ.items() if not k.startswith("OVS_POSE_")}
    d = tmp_path_factory.mktemp("pose_forms")
    res = {}
    for tag, (env, names) in _FORMS.items():
        f = str(d / (tag + ".npz"))
        subprocess.run([sys.executable, "-c", _CHILD, f] + list(names), env=dict(base, **env), timeout=120, check=True)
        with np.load(f) as z:
            res[tag] = {k: z[k] for k in z.files}
        assert sorted(res[tag]) == sorted(names)
    return res


@pytest.fixture(scope="module")
def default_forms():
    """name -> the in-process (default form) result, computed once: the second call of a frame must give the same bits."""
    assert not [k for k in os.environ if k.startswith("OVS_POSE_")], "the default forms need the default switches"
    from openvslam_amd import ba
    cache = {}

    def get(name):
        if name not in cache:
            frame = ps.frame_by_name(name)
            cache[name] = ps.run(ba, frame)
            again = ps.run(ba, frame)
            assert all(np.array_equal(a, b) for a, b in zip(cache[name], again)), name
        return cache[name]
    return get


def _check_against_oracle(oracle, frame, T, out, nv):
    wT, wout, wnv = ps.reference(oracle, frame)
    print("%s: |T - oracle| = %.3e, flags differing %d, nv %d / %d" % (frame.name, np.abs(T - wT).max(), int((out != (wout != 0)).sum()), nv, wnv))
    assert np.allclose(T, wT, rtol=0, atol=ps.TOL[frame.model]), np.abs(T - wT).max()
    assert np.array_equal(out, wout != 0) and nv == wnv
    if frame.name.startswith("perfect"):       # (the oracle itself moves by an ulp on three of the four: tests/test_pose_scenes.py)
        assert np.abs(T - frame.T0).max() <= 1e-15
    if frame.name.startswith("zero_weights"):
        assert np.array_equal(T, frame.T0)


@pytest.mark.parametrize("name", _EDGE + _EXTRA + _SCENES)
def test_default_form_at_every_edge(oracle, default_forms, name):
    """What the host entry selects by itself: 1 / 2 / 4 / 8 workgroups from 500 / 850 / 1600 observations, records in registers up to
    2 * groups * 256 of them and re-read from memory above (4097 and more)."""
    frame = ps.frame_by_name(name)
    _check_against_oracle(oracle, frame, *default_forms(name))


@pytest.mark.parametrize("tag,name", _FORM_CASES, ids=["%s-%s" % c for c in _FORM_CASES])
def test_forced_form(oracle, forced_forms, default_forms, tag, name):
    """Every form the switches can select, against the oracle; the from-memory form changes the data path only and must give the default form's
    bits."""
    frame = ps.frame_by_name(name)
    got = forced_forms[tag][name]
    _check_against_oracle(oracle, frame, *ps.unpack(got))
    if tag == "from_memory":
        assert np.array_equal(got, ps.pack(*default_forms(name)))


_BATCH_SIZES = (0, 4, 5, 63, 300, 513, 2600, 8192)


def _batch_frame(model, n):
    if n < 5:       # too short to optimise: any frame will do
        return ps.make(ps.Row(model, n, 90 + n, stereo_frac=0.5))
    return ps.frame_by_name(("p%d" if model == "persp" else "e%d") % n)


def _run_batch(model, frames):
    """frames through ovs_pose_optimize_batch_dev / ovs_pose_optimize_equirect_batch_dev: (poses [B, 12], flags, num_valid, offsets, input
    poses [B, 12]); the outputs are pre-filled with sentinels (777.0, 0xAB, -99)."""
    import ctypes as C
    import torch
    from openvslam_amd import _lib, ba
    L = _lib.lib()
    obs = np.concatenate([f.obs for f in frames])
    offs = np.cumsum([0] + [len(f.obs) for f in frames]).astype(np.int32)
    T_in = np.stack([np.concatenate([f.T0[:, :3].ravel(), f.T0[:, 3]]) for f in frames])   # R row-major | t
    d_T = torch.from_numpy(T_in).cuda()
    d_obs = torch.from_numpy(obs.view(np.uint8).copy()).cuda()
    d_off = torch.from_numpy(offs).cuda()
    d_out = torch.full_like(d_T, 777.0)
    d_fl = torch.full((max(len(obs), 1),), 0xAB, dtype=torch.uint8, device="cuda")
    d_nv = torch.full((len(frames),), -99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if model == "persp":
        st = L.ovs_pose_optimize_batch_dev(d_T.data_ptr(), d_obs.data_ptr(), d_off.data_ptr(), len(frames), C.byref(ba.BaCam(*frames[0].cam)),
                                           float(frames[0].bf), 1, d_out.data_ptr(), d_fl.data_ptr(), d_nv.data_ptr(), None)
    else:
        st = L.ovs_pose_optimize_equirect_batch_dev(d_T.data_ptr(), d_obs.data_ptr(), d_off.data_ptr(), len(frames), int(frames[0].cam[0]),
                                                    int(frames[0].cam[1]), d_out.data_ptr(), d_fl.data_ptr(), d_nv.data_ptr(), None)
    assert st == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_fl.cpu().numpy(), d_nv.cpu().numpy(), offs, T_in


@pytest.mark.parametrize("model", ["persp", "equirect"])
def test_batch_form(oracle, forced_forms, model):
    """One launch, one 256-thread workgroup per frame, frames of 0 to 8192 observations side by side (a mono-only frame next to an all-stereo one
    that is shorter than a workgroup: the kernel finds out per frame whether there is a stereo edge). Per frame against the oracle; and the
    same bits as the one-frame entry forced to one 256-thread workgroup: the same thread-to-observation assignment and the same reduction tree
    (that entry's registers-for-records and batched retries change no arithmetic)."""
    frames = [_batch_frame(model, n) for n in _BATCH_SIZES]
    assert [len(f.obs) for f in frames] == list(_BATCH_SIZES)
    if model == "persp":
        assert not frames[2].obs["is_stereo"].any() and frames[3].obs["is_stereo"].all()
    out, fl, nv, offs, T_in = _run_batch(model, frames)
    for k, f in enumerate(frames):
        n = len(f.obs)
        flags = fl[offs[k]:offs[k + 1]]
        if n < 5:
            assert nv[k] == 0 and np.array_equal(out[k], T_in[k]) and not flags.any()
            continue
        assert set(np.unique(flags)) <= {0, 1}
        T = np.concatenate([out[k][:9].reshape(3, 3), out[k][9:, None]], 1)
        _check_against_oracle(oracle, f, T, flags != 0, int(nv[k]))
        assert np.array_equal(ps.pack(T, flags, nv[k]), forced_forms["one_group_256"][f.name]), f.name
        if n == 8192:       # the last 256 observations: bit 31 of every thread's inlier mask
            wout = ps.reference(oracle, f)[1]
            assert wout[-256:].sum() >= 20 and np.array_equal(flags[-256:], wout[-256:])


def test_batch_refuses_an_over_long_frame(oracle):
    """A frame of more than 8192 observations does not fit the per-thread inlier mask: the batch entry reports -1 for it and touches neither its
    pose nor its flags; its neighbours are computed as without it. The one-frame entry returns OVS_ERR_CAPACITY."""
    from openvslam_amd import _lib, ba
    a, c = ps.frame_by_name("p300"), ps.make(ps.Row("persp", 300, 301, stereo_frac=0.4))
    long = ps.make(ps.Row("persp", 8193, 8193, stereo_frac=0.4))
    out, fl, nv, offs, _ = _run_batch("persp", [a, long, c])
    ref_out, ref_fl, ref_nv, ref_offs, _ = _run_batch("persp", [a, c])
    assert nv[1] == -1 and (out[1] == 777.0).all() and (fl[offs[1]:offs[2]] == 0xAB).all()
    for k, j in ((0, 0), (2, 1)):
        assert nv[k] == ref_nv[j] > 200 and np.array_equal(out[k], ref_out[j])
        assert np.array_equal(fl[offs[k]:offs[k + 1]], ref_fl[ref_offs[j]:ref_offs[j + 1]])
    T = np.concatenate([out[0][:9].reshape(3, 3), out[0][9:, None]], 1)
    _check_against_oracle(oracle, a, T, fl[:300] != 0, int(nv[0]))
    with pytest.raises(_lib.OvsError) as e:
        ps.run(ba, long)
    assert e.value.status == -4       # OVS_ERR_CAPACITY


@pytest.mark.parametrize("name", ["p499", "p500", "p1600", "p4097"])
def test_reset_each_round_variant_at_the_edges(oracle, default_forms, name):
    """Rule 25 (iv)'s variant on one, two and eight workgroups, records in registers and in memory, against the oracle's variant (the CPU side
    holds these rows to the same permutation-spread condition under the variant)."""
    from openvslam_amd import ba
    frame = ps.frame_by_name(name)
    try:
        ba.pose_set_variant("reset_each_round", 1)
        oracle.pose_set_variant("reset_each_round", 1)
        T, out, nv = ps.run(ba, frame)
        wT, wout, wnv = ps.run(oracle, frame)
    finally:
        ba.pose_set_variant("reset_each_round", 0)
        oracle.pose_set_variant("reset_each_round", 0)
    print("%s: |T - oracle| = %.3e" % (name, np.abs(T - wT).max()))
    assert np.allclose(T, wT, rtol=0, atol=1e-9) and np.array_equal(out, wout != 0) and nv == wnv
    assert not np.array_equal(T, default_forms(name)[0])       # the variant ran ...
    assert np.array_equal(ps.run(ba, frame)[0], default_forms(name)[0])       # ... and the default is back
