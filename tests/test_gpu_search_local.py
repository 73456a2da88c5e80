"""tracking_module::search_local_landmarks on the device (k_observe_landmarks + the projection matcher, csrc/match_window.hip)
against the sequential reference tests/observe_ref.py, exactly: observable, reproj as uint64 bits, x_right and level as bits, assigned and
both counts -- through the host-array form, the resident-frame form (twice on one handle), the device-pointer form and with the optional
outputs left out; the edges m = 0, n = 0, nothing searched; the old two-step path; and the C++ class layer through test_search_shim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import observe_ref as ref
import observe_scenes as scenes
from test_observe_ref import CASES, check_scene_conditions, seed_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
RATIO = 0.8
SF, LSF = scenes.SCALE_FACTORS, scenes.LOG_SCALE_FACTOR


@pytest.fixture(scope="module")
def match():
    from openvslam_amd import match
    return match


@pytest.fixture(scope="module")
def world(oracle):
    """Every scene and its reference at both margins, computed once and shared."""
    out = {}
    for case in CASES:
        model, stereo, n, m = case
        sc = scenes.scene(model, n, m, seed_of(*case), stereo)
        out[case] = (sc, {margin: scenes.reference(oracle, ref, sc, margin, RATIO) for margin in (5.0, 20.0)})
    return out


def _lib_cam(sc):
    from openvslam_amd import _lib
    return scenes.cameras(sc, _lib.Camera, _lib.GridParams)


def _call(w, sc, frame, margin, fields=True):
    cam, gp = _lib_cam(sc)
    return w.search_local_landmarks(cam, gp, frame, None if frame is not sc.kps else sc.desc, sc.pose, sc.pos, sc.dmm, sc.nrm, sc.lm_desc, SF, LSF, margin,
                                    frm_stereo_x_right=sc.x_right if frame is sc.kps else None, frm_occupied=sc.occupied, lm_search=sc.search, fields=fields)


def _same(got, want, fields=True):
    assigned, num, observable, f = got
    assert np.array_equal(observable, want["observable"]) and np.array_equal(assigned, want["assigned"]) and num == want["num_matches"]
    assert int(observable.sum()) == want["num_observable"]
    if fields:
        assert f["num_observable"] == want["num_observable"]
        assert np.array_equal(f["reproj"].view(np.uint64), want["reproj"].view(np.uint64))
        assert np.array_equal(f["x_right"].view(np.uint32), want["x_right"].view(np.uint32))
        assert np.array_equal(f["level"].view(np.uint32), want["level"].view(np.uint32))
    else:
        assert f is None


@pytest.mark.parametrize("margin", [5.0, 20.0])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_host_resident_and_optional_forms_equal_the_reference(match, oracle, world, case, margin):
    sc, refs = world[case]
    want = refs[margin]
    if sc.m >= 256:
        check_scene_conditions(oracle, sc, want, margin)
    w = match.projection(RATIO, True, max_targets=4096, max_queries=4096)
    _same(_call(w, sc, sc.kps, margin), want)
    _, gp = _lib_cam(sc)
    fd = match.frame_dev(gp, sc.kps, sc.desc, sc.x_right)
    for _ in range(2):   # the frame resident: twice on one handle
        _same(_call(w, sc, fd, margin), want)
    _same(_call(w, sc, sc.kps, margin, fields=False), want, fields=False)   # optional outputs NULL: not copied down
    _same(_call(w, sc, fd, margin, fields=False), want, fields=False)


@pytest.mark.parametrize("case", [(0, True, 2000, 3000), (1, False, 300, 257), (0, False, 300, 65)], ids=str)
def test_dev_form_equals_the_host_form_array_by_array(match, world, case):
    """ovs_tracking_search_local_landmarks_dev: every array in HBM, the caller's stream; with and without the optional outputs."""
    import torch
    from openvslam_amd import _lib
    L = _lib.lib()
    sc, refs = world[case]
    margin = 5.0
    w = match.projection(RATIO, True, max_targets=4096, max_queries=4096)
    assigned, num, observable, f = _call(w, sc, sc.kps, margin)
    _same((assigned, num, observable, f), refs[margin])
    dev = torch.device("cuda:0")
    keep = []

    def up(a):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev)
        keep.append(t)
        return t.data_ptr()

    cam, gp = _lib_cam(sc)
    pose = np.ascontiguousarray(np.concatenate([sc.pose[:, :3].reshape(-1), sc.pose[:, 3]]))
    ins = (up(sc.kps), up(sc.desc), up(sc.x_right), up(sc.occupied), sc.n, pose.ctypes.data, up(sc.pos), up(sc.dmm), up(sc.nrm), up(sc.lm_desc), up(sc.search),
           sc.m, SF.ctypes.data, len(SF), LSF, margin, RATIO)
    for optional in (True, False):
        d_obs = torch.full((sc.m,), 7, dtype=torch.uint8, device=dev)
        d_reproj = torch.full((sc.m, 2), -7.0, dtype=torch.float64, device=dev)
        d_xr = torch.full((sc.m,), -7.0, dtype=torch.float32, device=dev)
        d_lvl = torch.full((sc.m,), -7, dtype=torch.int32, device=dev)
        d_assigned = torch.full((sc.m,), -7, dtype=torch.int32, device=dev)
        d_nobs = torch.full((1,), -7, dtype=torch.int32, device=dev)
        d_num = torch.full((1,), -7, dtype=torch.int32, device=dev)
        opt = (d_reproj.data_ptr(), d_xr.data_ptr(), d_lvl.data_ptr()) if optional else (None, None, None)
        _lib.check(L.ovs_tracking_search_local_landmarks_dev(w._h, C.byref(cam), C.byref(gp), *ins, d_obs.data_ptr(), *opt, d_assigned.data_ptr(),
                                                             d_nobs.data_ptr(), d_num.data_ptr(), None), "ovs_tracking_search_local_landmarks_dev")
        torch.cuda.synchronize()
        assert int(d_num.cpu()[0]) == num and int(d_nobs.cpu()[0]) == f["num_observable"]
        assert np.array_equal(d_obs.cpu().numpy(), observable) and np.array_equal(d_assigned.cpu().numpy(), assigned)
        if optional:
            assert np.array_equal(d_reproj.cpu().numpy().view(np.uint64), f["reproj"].view(np.uint64))
            assert np.array_equal(d_xr.cpu().numpy().view(np.uint32), f["x_right"].view(np.uint32))
            assert np.array_equal(d_lvl.cpu().numpy(), f["level"])
        else:   # untouched
            assert (d_reproj.cpu().numpy() == -7.0).all() and (d_xr.cpu().numpy() == -7.0).all() and (d_lvl.cpu().numpy() == -7).all()
        _same(_call(w, sc, sc.kps, margin), refs[margin])   # the host form on the same context right behind the device form


def test_edges_no_landmarks_no_keypoints_nothing_searched_and_tight_capacity(match, oracle, world):
    sc, refs = world[(0, True, 300, 257)]
    w = match.projection(RATIO, True, max_targets=sc.n, max_queries=sc.m)   # a context of exactly this size: the staging arena holds the call
    _same(_call(w, sc, sc.kps, 5.0), refs[5.0])
    _, gp = _lib_cam(sc)
    fd = match.frame_dev(gp, sc.kps, sc.desc, sc.x_right)
    # m = 0: OK, both counts 0
    none = scenes.scene(0, 300, 0, 1, True)
    none.kps, none.desc, none.x_right, none.occupied = sc.kps, sc.desc, sc.x_right, sc.occupied
    for frame in (sc.kps, fd):
        assigned, num, observable, f = _call(w, none, frame, 5.0)
        assert num == 0 and f["num_observable"] == 0 and len(assigned) == len(observable) == 0
    # n = 0: the visibility alone, every assigned -1
    blind = scenes.scene(0, 0, 100, 2)
    want = scenes.reference(oracle, ref, blind, 5.0, RATIO)
    assert want["num_observable"] > 20 and want["num_matches"] == 0
    _same(_call(w, blind, blind.kps, 5.0), want)
    _same(_call(w, blind, blind.kps, 5.0, fields=False), want, fields=False)
    # nothing searched: 0 observable, 0 matches, the defined values
    idle = scenes.scene(0, 300, 257, seed_of(0, True, 300, 257), True)
    idle.search[:] = 0
    want = scenes.reference(oracle, ref, idle, 5.0, RATIO)
    assert want["num_observable"] == want["num_matches"] == 0
    for frame in (idle.kps, fd):
        _same(_call(w, idle, frame, 5.0), want)
    # and the context still serves the full scene
    _same(_call(w, sc, fd, 5.0), refs[5.0])
    from openvslam_amd import _lib
    with pytest.raises(_lib.OvsError) as e:   # one landmark more than the context holds
        big = scenes.scene(0, 300, 258, 3, True)
        _call(w, big, big.kps, 5.0)
    assert e.value.status == -4


@pytest.mark.parametrize("case", [(0, True, 2000, 3000), (1, False, 2000, 3000), (0, False, 300, 256)], ids=str)
def test_equals_the_old_two_step_path(match, world, case):
    """The reference's visibility fed to the library's existing match_frame_and_landmarks gives the same assigned as the one call."""
    sc, refs = world[case]
    _, gp = _lib_cam(sc)
    w = match.projection(RATIO, True, max_targets=4096, max_queries=4096)
    for margin in (5.0, 20.0):
        want = refs[margin]
        old, old_n = w.match_frame_and_landmarks(gp, sc.kps, sc.desc, SF, want["reproj"].astype(np.float32), want["level"], sc.lm_desc, margin,
                                                 frm_stereo_x_right=sc.x_right, frm_occupied=sc.occupied,
                                                 lm_x_right=want["x_right"] if sc.x_right is not None else None, lm_valid=want["observable"])
        new, new_n, _, _ = _call(w, sc, sc.kps, margin, fields=False)
        assert old_n == new_n == want["num_matches"] and np.array_equal(old, new)


@pytest.mark.parametrize("case", [(0, True, 300, 257), (1, False, 300, 256)], ids=str)
def test_cpp_class_layer(tmp_path, oracle, case):
    """module::search_local_landmarks through test_search_shim: frm.landmarks_, the observable flags, the num_observable_ increments of both
    loops, and the tracking fields with write_tracking_fields on. The frame already holds some landmarks (they are not searched again) and
    some local landmarks are about to be erased."""
    model, stereo, n, m = case
    sc = scenes.scene(model, n, m, seed_of(*case), stereo)
    sc.focal_x_baseline = float(np.float32(sc.focal_x_baseline))   # camera::base::focal_x_baseline_ is a float
    rng = np.random.default_rng(9)
    held_lms = rng.choice(m, 24, replace=False)
    held = {int(k): int(l) for k, l in zip(rng.choice(n, 24, replace=False), held_lms)}   # curr_frm.landmarks_[k] = local_landmarks[l]
    erased = {int(l) for l in rng.choice(m, 12, replace=False)}
    frame_id = 41
    # what the shim has to flatten: V1 from the object graph, occupied from the held landmarks (all of them have observations)
    sc.search = np.array([0 if (l in erased or l in held.values()) else 1 for l in range(m)], np.uint8)
    sc.occupied = np.zeros(n, np.uint8)
    sc.occupied[list(held)] = 1
    want = scenes.reference(oracle, ref, sc, 5.0, RATIO)
    assert want["num_matches"] > n // 20 and want["num_observable"] > want["num_matches"]
    cpp = os.path.join(ROOT, "openvslam_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp] + (["asan"] if SUFFIX else ["test_search_shim"]))
    scenes.write_scene(tmp_path / "scene.bin", sc, 5.0, RATIO, frame_id, held, erased)
    r = subprocess.run([os.path.join(cpp, "test_search_shim" + SUFFIX), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ABI calls failed 0" in r.stdout, r.stdout + r.stderr
    expect_held = np.full(n, -1, np.int32)
    for k, l in held.items():
        expect_held[k] = l
    for l in np.nonzero(want["assigned"] >= 0)[0]:
        expect_held[want["assigned"][l]] = l
    first_loop = np.array([1 if (l in held.values() and l not in erased) else 0 for l in range(m)])
    for run, fields in zip(scenes.read_results(tmp_path / "out.bin", n, m), (False, True)):
        assert run["num_matches"] == want["num_matches"] and np.array_equal(run["landmarks"], expect_held)
        lms = run["lms"]
        assert np.array_equal(lms["observable"], want["observable"])
        assert np.array_equal(lms["num_observable"], 1 + first_loop + want["observable"])   # num_observable_ starts at 1
        if fields:
            assert np.array_equal(lms["reproj"].view(np.uint64), want["reproj"].view(np.uint64))
            assert np.array_equal(lms["x_right"].view(np.uint32), want["x_right"].view(np.uint32)) and np.array_equal(lms["level"], want["level"])
        else:   # the fields keep the values the landmarks were constructed with
            assert not lms["reproj"].any() and (lms["x_right"] == -1.0).all() and not lms["level"].any()
