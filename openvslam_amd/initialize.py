"""initialize::perspective (expected: src/openvslam/initialize/{base,perspective}.{h,cc}) on the MI355X: the monocular initialiser's
two-view geometry as two device calls. initialize() hands the matched keypoints to solve.solve_two_view_batch (the H and the F RANSAC and
the choice between them) and the chosen model to solve.reconstruct_two_view_batch (its pose hypotheses, check_pose and
find_most_plausible_pose); no loop over matches runs on the host."""
import numpy as np

from . import solve


class perspective:
    """Upstream's constructor (ref_frm, num_ransac_iters, min_num_triangulated, parallax_deg_thr, reproj_err_thr), initialize() and the four
    getters. ref_frm: a dict with undist_keypts (n, 2), bearings (n, 3) and camera (solve.camera, perspective). The results are indexed by
    the reference frame's keypoints, as upstream stores them."""

    def __init__(self, ref_frm, num_ransac_iters=100, min_num_triangulated=50, parallax_deg_thr=1.0, reproj_err_thr=4.0, seed=solve.TWO_VIEW_DEFAULT_SEED,
                 device=0):
        self._ref_keypts = np.asarray(ref_frm["undist_keypts"], np.float64).reshape(-1, 2)
        self._ref_bearings = np.asarray(ref_frm["bearings"], np.float64).reshape(-1, 3)
        self._cam = ref_frm["camera"]
        self._iters, self._min_num, self._parallax, self._reproj = int(num_ransac_iters), int(min_num_triangulated), float(parallax_deg_thr), float(reproj_err_thr)
        self._seed, self._device = seed, device
        self._two_view_handle = self._reconstruct_handle = None
        self._clear()

    def _clear(self):
        n = len(self._ref_keypts)
        self._rot, self._trans = np.zeros((3, 3)), np.zeros(3)
        self._pts, self._flags = np.zeros((n, 3)), np.zeros(n, bool)

    def _handles(self, m):
        if self._two_view_handle is None or self._two_view_handle.max_total_matches < m:
            self._two_view_handle = solve._two_view_handle(1, max(m, 1), self._device)
            self._reconstruct_handle = solve._reconstruct_handle(1, max(m, 1), self._device)
        return self._two_view_handle, self._reconstruct_handle

    def initialize(self, cur_undist_keypts, cur_bearings, ref_matches_with_cur):
        """ref_matches_with_cur[i]: the current frame's keypoint matched to reference keypoint i, or -1. True where the map can be built."""
        self._clear()
        matches = np.asarray(ref_matches_with_cur, np.int64).ravel()
        ref_idx = np.nonzero(matches >= 0)[0]
        cur_idx = matches[ref_idx]
        cur_keypts = np.asarray(cur_undist_keypts, np.float64).reshape(-1, 2)
        two_view = dict(x1=self._ref_keypts[ref_idx], x2=cur_keypts[cur_idx])
        two_view_handle, reconstruct_handle = self._handles(len(ref_idx))
        solution = solve.solve_two_view_batch([two_view], 1.0, self._iters, True, self._seed, handle=two_view_handle, device=self._device)[0]
        problem = solve.reconstruct_problem_from_solution(solution, two_view, self._cam, self._ref_bearings[ref_idx],
                                                          np.asarray(cur_bearings, np.float64).reshape(-1, 3)[cur_idx])
        if problem is None:
            return False
        r = solve.reconstruct_two_view_batch([problem], self._reproj, self._parallax, self._min_num, handle=reconstruct_handle, device=self._device)[0]
        if not r["success"]:
            return False
        self._rot, self._trans = r["rot_ref_to_cur"], r["trans_ref_to_cur"]
        self._pts[ref_idx], self._flags[ref_idx] = r["triangulated_pts"], r["is_triangulated"]
        return True

    def get_rotation_ref_to_cur(self):
        return self._rot

    def get_translation_ref_to_cur(self):
        return self._trans

    def get_triangulated_pts(self):
        return self._pts

    def get_triangulated_flags(self):
        return self._flags
