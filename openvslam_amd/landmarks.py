"""Landmark upkeep on the device (csrc/landmark_update.hip; DESIGN.md 3.14, rules L1 to L9): data::landmark::update_normal_and_depth and
data::landmark::compute_descriptor (expected: src/openvslam/data/landmark.cc) for many landmarks in one call -- the mean viewing normal,
the raw valid distance range and the representative descriptor that every matcher which takes landmarks reads. `landmark_updater.update` is the
C ABI's arrays; `update_map` is the step a caller adds after `io.load_map_database`, which stores none of the three."""
import ctypes as C

import numpy as np

from . import _lib

GEOMETRY, DESCRIPTOR, BOTH = 1, 2, 3
MAX_LANDMARKS_PER_CALL = 65535


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def scale_factors_of(scale_factor, num_levels):
    """orb_params::scale_factors_: scale_factors_[l] = scale_factor * scale_factors_[l - 1] in float."""
    out, sf = [], np.float32(1.0)
    for _ in range(int(num_levels)):
        out.append(sf)
        sf = np.float32(np.float32(scale_factor) * sf)
    return np.array(out, np.float32)


def cam_center_of(rot_cw, trans_cw):
    """keyframe::get_cam_center: -R^T t of the stored quaternion (x, y, z, w) and translation, world -> camera."""
    x, y, z, w = (float(v) for v in rot_cw)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    t = np.asarray(trans_cw, np.float64)
    return np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)])


class landmark_updater:
    """One handle (ovs_landmarks): up to max_landmarks landmarks (at most 65535) of max_total_observations observations together per call, in
    up to max_keyframes keyframes."""

    def __init__(self, device=0, max_landmarks=MAX_LANDMARKS_PER_CALL, max_total_observations=1 << 20, max_keyframes=4096):
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.ovs_landmarks_create(device, max_landmarks, max_total_observations, max_keyframes, C.byref(h)), "ovs_landmarks_create")
        self._h = h
        self.device, self.max_landmarks, self.max_total_observations, self.max_keyframes = device, max_landmarks, max_total_observations, max_keyframes

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.ovs_landmarks_destroy(h)

    def update(self, what, offsets, pos_w, ref_keyfrm, ref_level, obs_keyfrm, obs_desc=None, frame_devs=None, obs_keypoint=None, obs_use=None, cam_centers=None,
               scale_factors=None, out=None):
        """The C ABI's call. Either obs_desc (T x 32 bytes) or frame_devs (a match.frame_dev per keyframe slot) with obs_keypoint (T). Returns the
        five outputs as a dict: mean_normal (n, 3) f64, min_max_dist (n, 2) f32, best_obs (n,) i32, desc (n, 32) u8, status (n,) u8. What a
        rule leaves untouched keeps the value of `out` (a dict of the same arrays), or zero (best_obs: -1) without one."""
        arr = lambda a, t, shape: None if a is None else np.ascontiguousarray(a, t).reshape(shape)
        offsets = arr(offsets, np.int32, -1)
        n = len(offsets) - 1
        pos_w, ref_keyfrm, ref_level = arr(pos_w, np.float64, (-1, 3)), arr(ref_keyfrm, np.int32, -1), arr(ref_level, np.int32, -1)
        obs_keyfrm, obs_use = arr(obs_keyfrm, np.int32, -1), arr(obs_use, np.uint8, -1)
        cam_centers, scale_factors = arr(cam_centers, np.float64, (-1, 3)), arr(scale_factors, np.float32, -1)
        K = len(cam_centers) if cam_centers is not None else (len(frame_devs) if frame_devs is not None else 0)
        if out is None:
            out = dict(mean_normal=np.zeros((n, 3)), min_max_dist=np.zeros((n, 2), np.float32), best_obs=np.full(n, -1, np.int32), desc=np.zeros((n, 32), np.uint8),
                       status=np.zeros(n, np.uint8))
        head = (self._h, int(what), n, _p(offsets), _p(pos_w), _p(ref_keyfrm), _p(ref_level), _p(obs_keyfrm))
        tail = (_p(obs_use), _p(cam_centers), K, _p(scale_factors), 0 if scale_factors is None else len(scale_factors), _p(out["mean_normal"]), _p(out["min_max_dist"]),
                _p(out["best_obs"]), _p(out["desc"]), _p(out["status"]))
        if frame_devs is not None:
            handles = (C.c_void_p * max(len(frame_devs), 1))(*[f._h.value for f in frame_devs])
            _lib.check(self._L.ovs_landmarks_update_batch_f(*head, handles, _p(arr(obs_keypoint, np.int32, -1)), *tail), "ovs_landmarks_update_batch_f")
        else:
            _lib.check(self._L.ovs_landmarks_update_batch(*head, _p(arr(obs_desc, np.uint8, (-1, 32))), *tail), "ovs_landmarks_update_batch")
        return out

    def update_map(self, db, landmark_ids=None, what=BOTH):
        """update_normal_and_depth and compute_descriptor for the landmarks of an io.map_database (all of them, or landmark_ids): the observations
        in the order of db.observations(), in chunks of at most 65535 landmarks. Stores descriptor, mean_normal, min_valid_dist and max_valid_dist
        on the io.landmark objects (a landmark without observations keeps what it had) and returns the number of landmarks updated."""
        ids = sorted(db.landmarks) if landmark_ids is None else [int(i) for i in landmark_ids]
        if not ids:
            return 0
        obs = db.observations()
        kf_ids = sorted(db.keyframes)
        slot = {k: i for i, k in enumerate(kf_ids)}
        tables = {(float(np.float32(kf.scale_factor)), int(kf.n_scale_levels)) for kf in db.keyframes.values()}
        if len(tables) != 1:
            raise ValueError("keyframes with different scale tables in one call: %s" % sorted(tables))
        scale_factors = scale_factors_of(*next(iter(tables)))
        centres = np.array([cam_center_of(db.keyframes[k].rot_cw, db.keyframes[k].trans_cw) for k in kf_ids]).reshape(-1, 3)
        updated = 0
        for at in range(0, len(ids), min(self.max_landmarks, MAX_LANDMARKS_PER_CALL)):
            chunk = ids[at:at + min(self.max_landmarks, MAX_LANDMARKS_PER_CALL)]
            offsets, pos, ref_kf, ref_lv, o_kf, o_desc = [0], [], [], [], [], []
            for lid in chunk:
                lm, mine = db.landmarks[lid], obs[lid]
                level = 0
                if mine:
                    where = [idx for kid, idx in mine if kid == lm.ref_keyfrm]
                    if not where:
                        raise ValueError("landmark %d: its reference keyframe %d does not observe it" % (lid, lm.ref_keyfrm))
                    level = int(db.keyframes[lm.ref_keyfrm].keypts["octave"][where[0]])
                for kid, idx in mine:
                    o_kf.append(slot[kid])
                    o_desc.append(db.keyframes[kid].descs[idx])
                offsets.append(len(o_kf))
                pos.append(lm.pos_w)
                ref_kf.append(slot[lm.ref_keyfrm] if mine else 0)
                ref_lv.append(level)
            r = self.update(what, offsets, pos, ref_kf, ref_lv, o_kf, obs_desc=np.array(o_desc, np.uint8).reshape(-1, 32), cam_centers=centres,
                            scale_factors=scale_factors)
            for i, lid in enumerate(chunk):
                if r["status"][i] != 0:
                    continue
                lm = db.landmarks[lid]
                if what & GEOMETRY:
                    lm.mean_normal = r["mean_normal"][i].copy()
                    lm.min_valid_dist, lm.max_valid_dist = float(r["min_max_dist"][i, 0]), float(r["min_max_dist"][i, 1])
                if what & DESCRIPTOR and r["best_obs"][i] >= 0:
                    lm.descriptor = r["desc"][i].copy()
                updated += 1
        return updated
