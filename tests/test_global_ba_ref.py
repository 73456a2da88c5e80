"""Global bundle adjustment, the part that needs no device: the graph io.global_ba_problem flattens from a map, and the CPU restatement of
the whole call (tests/global_ba_ref.py: the oracle's Levenberg-Marquardt around the reference conjugate gradient) against the oracle."""
import numpy as np

import global_ba_ref


def _tiny_map():
    """Three keyframes (0, 1, 2) and one to be erased (3); landmarks 10, 11, 12, one to be erased (13) and one nobody observes (14)."""
    from openvslam_amd import io
    from openvslam_amd.match import KP_DTYPE
    db = io.map_database()
    db.cameras = {"cam": {"model_type": "Perspective", "setup_type": "Stereo", "fx": 500.0, "fy": 510.0, "cx": 320.0, "cy": 240.0,
                          "focal_x_baseline": 40.0, "cols": 640, "rows": 480}}
    lm_of = {0: [10, 11, -1], 1: [11, 12, 13], 2: [12, 10, 11], 3: [10, 12, 13]}
    for k, lms in lm_of.items():
        n = len(lms)
        kp = np.zeros(n, KP_DTYPE)
        kp["octave"] = [0, 1, 2]
        kp["x"] = kp["y"] = 0
        db.keyframes[k] = io.keyframe(id=k, rot_cw=np.array([0.0, 0.0, 0.0, 1.0]), trans_cw=np.array([0.1 * k, 0.0, 0.0]), keypts=kp,
                                      undists=np.array([[100.0 * k + i, 50.0 + i] for i in range(n)], np.float32),
                                      x_rights=np.array([-1.0, 90.0 + k, -1.0], np.float32), depths=np.full(n, -1.0, np.float32),
                                      descs=np.zeros((n, 32), np.uint8), lm_ids=np.array(lms, np.int64))
    for j in (10, 11, 12, 13, 14):
        db.landmarks[j] = io.landmark(id=j, first_keyfrm=0, pos_w=np.array([0.01 * j, 0.02 * j, 5.0]), ref_keyfrm=0)
    db.keyframes[3].will_be_erased = True
    db.landmarks[13].will_be_erased = True
    return io, db


def test_global_ba_problem_against_hand_written_lists():
    """R4: keyframes and landmarks that are not to be erased, keyframe 0 fixed, the edges landmark by landmark in ascending keyframe id."""
    io, db = _tiny_map()
    p = io.global_ba_problem(db)
    assert p["keyfrm_ids"] == [0, 1, 2] and p["lm_ids"] == [10, 11, 12]
    assert p["pose_fixed"].tolist() == [1, 0, 0]
    assert np.array_equal(p["poses"][:, 0], [0.0, 0.1, 0.2]) and np.array_equal(p["poses"][:, 3:], [[0, 0, 0, 1]] * 3)
    assert np.array_equal(p["points"], [[0.10, 0.20, 5.0], [0.11, 0.22, 5.0], [0.12, 0.24, 5.0]])
    w = io.inv_level_sigma_sq(1.2, 8)
    # keypoint 1 of every keyframe carries a right coordinate: those observations are stereo edges
    # landmark 10: keyframe 0 keypoint 0 (mono), keyframe 2 keypoint 1 (stereo); 11: kf 0 kp 1 (stereo), kf 1 kp 0 (mono), kf 2 kp 2 (mono);
    # 12: kf 1 kp 1 (stereo), kf 2 kp 0 (mono)
    want_mono = [(0, 0, 0.0, 50.0, w[0]), (1, 1, 100.0, 50.0, w[0]), (2, 1, 202.0, 52.0, w[2]), (2, 2, 200.0, 50.0, w[0])]
    want_stereo = [(2, 0, 201.0, 51.0, 92.0, w[1]), (0, 1, 1.0, 51.0, 90.0, w[1]), (1, 2, 101.0, 51.0, 91.0, w[1])]
    assert [tuple(e) for e in p["mono"].tolist()] == want_mono
    assert [tuple(e) for e in p["stereo"].tolist()] == want_stereo
    assert p["cam"].tolist() == [500.0, 510.0, 320.0, 240.0] and p["focal_x_baseline"] == 40.0 and p["setup_type"] == 1 and p["model"] == 0
    # an equirectangular rig has monocular edges only
    db.cameras["cam"]["model_type"] = "Equirectangular"
    q = io.global_ba_problem(db)
    assert len(q["stereo"]) == 0 and len(q["mono"]) == 7 and q["model"] == 1 and (q["cols"], q["rows"]) == (640, 480)
    assert [tuple(e)[:2] for e in q["mono"].tolist()] == [(0, 0), (2, 0), (0, 1), (1, 1), (2, 1), (1, 2), (2, 2)]


def test_restatement_reproduces_the_oracles_first_round(oracle):
    """R5: the oracle's local_ba_optimize(num_first_iter = 10, num_second_iter = 0) on the 24-keyframe ring, within 1e-9. Found: keyframes
    3.6e-13, landmarks 2.2e-13; ten iterations, ten trials, 762 solver iterations in all."""
    from oracle import lba
    d, got = global_ba_ref.reference("ring24")
    want = lba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], None, 0.0, 10, 0)
    print("keyframes %.3g, landmarks %.3g, info %s" % (np.abs(got["poses"] - want["poses"]).max(), np.abs(got["points"] - want["points"]).max(), got["info"]))
    assert np.abs(got["poses"] - want["poses"]).max() <= 1e-9 and np.abs(got["points"] - want["points"]).max() <= 1e-9
    assert got["info"][2] == want["info"][4] == 10 and got["info"][3] == 10 and got["info"][5] == 0
    assert np.allclose(got["info"][:2], want["info"][:2], rtol=1e-9)
    assert np.array_equal(got["poses"][0], d["poses"][0])


def test_restatement_rejects_a_trial_on_the_gross_start(oracle):
    """R5: global_ba_ref.ring24_far (every landmark moved by N(0, 4.0), seed 77). Found: ten iterations, twelve trials."""
    d, got = global_ba_ref.reference("ring24_far")
    print(got["info"])
    assert got["info"][2] == 10 and got["info"][3] > got["info"][2] and got["info"][5] == 0
    assert got["info"][1] < got["info"][0]
