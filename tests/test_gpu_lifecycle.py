"""Resource lifetime behind the C ABI (csrc/owned_internal.inc): every handle gives back exactly what it acquired. The measure is
ovs_debug_live_resources(), the process-wide count of streams, events, device and page-locked blocks that any handle or per-thread work
space holds. Per-thread work spaces and the arena pools persist by design, so every comparison starts after one warm cycle."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_pnp as gp
import test_gpu_sim3 as gs
from test_ba import _lba_scene

pytestmark = pytest.mark.gpu

OK, ERR_HIP = 0, -3
ROWS, COLS, NFEAT = 240, 400, 500


@pytest.fixture(scope="module")
def m():
    """The modules, the library, and the inputs every cycle shares (built once)."""
    from types import SimpleNamespace
    from openvslam_amd import _lib, ba, bow, feature, match, solve, synth
    s = SimpleNamespace(L=_lib.lib(), lib=_lib, ba=ba, bow=bow, feature=feature, match=match, solve=solve, synth=synth)
    s.live = s.L.ovs_debug_live_resources
    s.left, s.right, _ = synth.synth_stereo_pair(ROWS, COLS, seed=3)
    s.mask = np.full((ROWS, COLS), 255, np.uint8)
    s.mask[:, :COLS // 4] = 0
    s.kps, s.desc = synth.synth_keypoints(64, ROWS, COLS, seed=5)
    s.grid = match.grid_params(COLS, ROWS)
    s.vocab = synth.synth_vocabulary(k=6, depth=3, seed=2)
    s.scene = _lba_scene(31, n_pose=9, n_pt=1200, obs_per_pose=400, stereo_frac=0.3)
    # the stereo matcher reads the pyramids of two extractors' last extract: they live as long as the module
    s.el, s.er = (feature.orb_extractor(feature.orb_params(NFEAT), max_rows=ROWS, max_cols=COLS) for _ in range(2))
    s.kl, s.dl = s.el.extract(s.left)
    s.kr, s.dr = s.er.extract(s.right)
    return s


def new_extractor(m, max_batch=1):
    return m.feature.orb_extractor(m.feature.orb_params(NFEAT), max_rows=ROWS, max_cols=COLS, max_batch=max_batch)


def multi_cycle(m, n_gpus):
    d, mono, st, bf, _, _ = m.scene
    if n_gpus > 1:   # (the sharded entry's own test runs mono edges only)
        st = st[:0]
    n_pose, n_pt = len(d["poses"]), len(d["points"])
    cam, h, fixed = m.ba.BaCam(*d["cam"]), C.c_void_p(), np.ascontiguousarray(d["pose_fixed"], np.uint8)
    m.lib.check(m.L.ovs_ba_multi_create(n_gpus, n_pose, fixed.ctypes.data, n_pt, mono.ctypes.data, len(mono), st.ctypes.data if len(st) else None,
                                        len(st), C.byref(cam), bf, C.byref(h)), "ovs_ba_multi_create")
    try:
        out = [np.zeros(n) for n in (36 * n_pose, 6 * n_pose, 9 * n_pt, 3 * n_pt, 18 * (len(mono) + len(st)), 2)]
        P, X = np.ascontiguousarray(d["poses"]), np.ascontiguousarray(d["points"])
        m.lib.check(m.L.ovs_ba_multi_linearize(h, P.ctypes.data, X.ctypes.data, 2.0, 2.5, *[o.ctypes.data for o in out]), "ovs_ba_multi_linearize")
    finally:
        assert m.L.ovs_ba_multi_destroy(h) == OK


def cycle(m, kind):
    """create, one smallest valid call, destroy"""
    if kind == "orb":
        ex = new_extractor(m)
        ex.extract(m.left)
        ex.__del__()
    elif kind == "matcher":
        mt = m.match.robust(0.9, False, max_n1=128, max_n2=128)
        mt.brute_force_match(m.desc[:1], m.desc[:1])
        mt.__del__()
    elif kind == "wmatcher":
        w = m.match.projection(0.8, False, max_targets=4096, max_queries=16)
        w.assign_keypoints_to_grid(m.grid, m.kps[:1])
        w.__del__()
    elif kind == "frame_dev":
        f = m.match.frame_dev(m.grid, m.kps, m.desc)
        assert f.device == 0
        f.__del__()
    elif kind == "stereo":
        st = m.match.stereo(m.el, m.er, m.kl, m.dl, m.kr, m.dr, 386.1448, 0.5372, max_rows=ROWS, max_keypoints=max(len(m.kl), len(m.kr), 1))
        st.compute()
        st.__del__()
    elif kind == "vocab":
        v = m.bow.vocabulary(m.vocab, max_features=16)
        v.transform_features(m.desc[:1], 4)
        v.__del__()
    elif kind == "bowdb":
        db = m.bow.bow_database(4, max_words=8)
        db.add_keyframe(1, {2: .5, 7: .5})
        db.score_all({2: 1.0})
        db.__del__()
    elif kind == "sim3":
        h = m.solve._handle(1, 70)
        gs.run(m.solve, "n3", handle=h)
        h.__del__()
    elif kind == "pnp":
        h = m.solve._pnp_handle(1, 70)
        gp.run(m.solve, "n4", handle=h)
        h.__del__()
    elif kind == "ba_graph":
        import torch
        d, mono, st, bf, _, _ = m.scene
        g = m.ba.graph(len(d["poses"]), d["pose_fixed"], len(d["points"]), mono, d["cam"], st, bf)
        g.linearize_dev(torch.from_numpy(d["poses"]).cuda(), torch.from_numpy(d["points"]).cuda(), 2.0, 2.5)
        torch.cuda.synchronize()
        g.__del__()
    elif kind == "ba_multi_1":
        multi_cycle(m, 1)
    else:
        assert kind == "ba_multi_2"
        multi_cycle(m, 2)


@pytest.mark.parametrize("kind", ["orb", "matcher", "wmatcher", "frame_dev", "stereo", "vocab", "bowdb", "sim3", "pnp", "ba_graph", "ba_multi_1", "ba_multi_2"])
def test_balanced(m, kind):
    """Four create / call / destroy cycles after a warm one leave the count exactly where it was."""
    if kind == "ba_multi_2" and m.L.ovs_device_count() < 2:
        pytest.skip("needs >= 2 HIP devices")
    cycle(m, kind)
    c0 = m.live()
    for _ in range(4):
        cycle(m, kind)
    assert m.live() == c0


def test_lazy_members_of_an_extractor(m):
    """Every path of ovs_orb that allocates late -- mask planes, the pair buffers, the host pyramid, the sub-batch streams, the per-slot timing
    events -- then destroy: the count is back where it was before the create. (The stage profilers' events are outside the count.)"""
    import torch
    before = m.live()
    ex = new_extractor(m, max_batch=2)
    created = m.live()
    assert created > before
    ex.extract(m.left, m.mask)
    ex.extract_pair(m.left, m.right, m.mask, m.mask)
    assert m.L.ovs_orb_set_host_pyramid(ex._h, 1) == OK
    ex.extract(m.left)
    ex.set_pipeline(2)
    cap = ex.max_keypoints
    d_img = torch.from_numpy(np.stack([m.left, m.right])).cuda()
    d_kps = torch.zeros((2, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    ex.extract_batch_dev(d_img, d_kps, d_desc, d_cnt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert m.L.ovs_orb_profile_enable(ex._h, 1) == OK
    ex.extract(m.left)
    assert m.live() > created   # the late allocations are counted ...
    ex.__del__()
    assert m.live() == before   # ... and given back


def test_matcher_with_its_profiler_and_a_refused_create(m):
    """A brute-force matcher whose stage profiler created its events (outside the count) gives back what the create took; a create the plan refuses
    (the one-wave resolver's LDS beyond 150 KiB) takes nothing and hands back no handle."""
    ERR_CAPACITY = -4
    before = m.live()
    mt = m.match.robust(0.9, False, max_n1=128, max_n2=128)
    assert m.live() > before
    assert m.L.ovs_matcher_profile_enable(mt._h, 1) == OK
    mt.brute_force_match(m.desc[:8], m.desc[:8])
    stage_ms, ncalls = (C.c_float * 2)(), C.c_int32()
    assert m.L.ovs_matcher_profile_read(mt._h, stage_ms, C.byref(ncalls)) == OK and ncalls.value == 1
    mt.__del__()
    assert m.live() == before
    h = C.c_void_p(1)
    assert m.L.ovs_matcher_create(30721, 1, 1, 0, C.byref(h)) == ERR_CAPACITY and not h.value and m.live() == before


def test_lazy_members_of_frame_and_solver_handles(m):
    """A frame handle with bearings attached, and a Sim3 and an EPnP handle whose models grew once (max_num_iter 257 / 65)."""
    cycle(m, "frame_dev")   # the calling thread's staging buffer and stream persist
    before = m.live()
    f = m.match.frame_dev(m.grid, m.kps, m.desc).attach_bearings(np.ones((len(m.kps), 3)))
    assert m.live() == before + 1
    f.__del__()
    assert m.live() == before
    for mod, handle in ((gs, m.solve._handle), (gp, m.solve._pnp_handle)):
        before = m.live()
        h = handle(1, 70)
        created = m.live()
        got = [mod.of_device(mod.run(m.solve, "n65_noisy", k, handle=h)) for k in (mod.ITERS, mod.GROW_ITERS)]
        assert got == [mod.of_reference(mod.expected("n65_noisy", k)) for k in (mod.ITERS, mod.GROW_ITERS)]
        assert m.live() == created   # the grown block replaced the first one
        h.__del__()
        assert m.live() == before


@pytest.mark.parametrize("kind", ["bowdb", "sim3", "pnp"])
def test_failed_creates_release_everything(m, kind):
    """The creates whose HIP calls pass through the failure injection: the k-th checked call reported as failed, for k = 0, 1, 2, ... until
    the create succeeds. Every failure returns OVS_ERR_HIP with *out == NULL and the count unchanged; a normal create and call afterwards
    give the existing tests' expected result. (The injection only changes what a finished HIP call reports.)"""
    create = {"bowdb": lambda out: m.L.ovs_bowdb_create(0, 4, 8, out), "sim3": lambda out: m.L.ovs_sim3_create(0, 1, 70, out),
              "pnp": lambda out: m.L.ovs_pnp_create(0, 1, 70, out)}[kind]
    destroy = getattr(m.L, "ovs_%s_destroy" % kind)
    c0, failures, h = m.live(), 0, C.c_void_p()
    try:
        for skip in range(64):
            h = C.c_void_p()
            m.L.ovs_debug_inject_hip_failures(skip, 1)
            rc = create(C.byref(h))
            if rc == OK:
                break
            assert rc == ERR_HIP and not h.value and m.live() == c0, (skip, rc, h.value, m.live(), c0)
            failures += 1
        else:
            pytest.fail("the create still fails with 64 checked calls skipped")
    finally:
        m.L.ovs_debug_inject_hip_failures(0, 0)
    assert h.value and m.live() > c0
    assert destroy(h) == OK and m.live() == c0
    assert failures >= 3
    if kind == "bowdb":
        db = m.bow.bow_database(4, max_words=8)
        db.add_keyframe(1, {2: .5, 7: .25, 9: .25})
        db.add_keyframe(2, {1: .5, 2: .25, 7: .25})
        db.add_keyframe(3, {3: 1.0})
        assert db.score_all({1: .5, 2: .25, 7: .25}) == [(1, 2, 0.5), (2, 3, 1.0), (3, 0, 0.0)]
    else:
        mod = gs if kind == "sim3" else gp
        assert mod.of_device(mod.run(m.solve, "n65")) == mod.of_reference(mod.expected("n65"))
