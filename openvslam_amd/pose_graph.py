"""optimize::graph_optimizer (expected: src/openvslam/optimize/graph_optimizer.{h,cc}) on the device: the Sim3 pose-graph optimisation over
the essential graph after an accepted loop and the landmark write-back, one call of two launches (rules G1 to G11; the C ABI
is ovs_posegraph_* of include/ovslam_hip.h). `optimize_arrays` is the C ABI with numpy arrays; `graph_optimizer` is upstream's class over the
problem `openvslam_amd.io.pose_graph_problem` builds from a map database."""
import ctypes as C

import numpy as np

from . import _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class graph_optimizer:
    """The constructor is upstream's (map_db is the problem's business here, so: fix_scale); one handle, grown when a problem outgrows it."""

    def __init__(self, fix_scale, device=0, max_vertices=256, max_edges=1024, max_landmarks=4096):
        self._fix_scale, self._device = bool(fix_scale), int(device)
        self._cap = (0, 0, 0)
        self._h = None
        self._reserve(max_vertices, max_edges, max_landmarks)

    def _reserve(self, n_v, n_e, n_l):
        want = (max(self._cap[0], n_v, 1), max(self._cap[1], n_e), max(self._cap[2], n_l))
        if self._h is not None and want == self._cap:
            return
        self.close()
        h = C.c_void_p()
        _lib.check(_lib.lib().ovs_posegraph_create(self._device, want[0], want[1], want[2], C.byref(h)), "ovs_posegraph_create")
        self._h, self._cap = h, want

    def close(self):
        if self._h is not None:
            _lib.lib().ovs_posegraph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def optimize_arrays(self, rot, trans, scale, fixed, nc_rot, nc_trans, nc_scale, edge_ij, edge_rot, edge_trans, edge_scale, lm_ref, lm_pos,
                        num_iter=50, pcg_max_iter=0, fix_scale=None):
        """The C ABI over numpy arrays. Returns (rot (n, 3, 3), trans (n, 3), scale (n), lm_pos (m, 3), info (8))."""
        f8 = lambda a, *shape: np.ascontiguousarray(a, np.float64).reshape(*shape)
        n_v, n_e, n_l = len(np.asarray(scale).reshape(-1)), len(np.asarray(edge_scale).reshape(-1)), len(np.asarray(lm_ref).reshape(-1))
        rot, trans, scale = f8(rot, n_v, 9), f8(trans, n_v, 3), f8(scale, n_v)
        nc_rot, nc_trans, nc_scale = f8(nc_rot, n_v, 9), f8(nc_trans, n_v, 3), f8(nc_scale, n_v)
        edge_rot, edge_trans, edge_scale = f8(edge_rot, n_e, 9), f8(edge_trans, n_e, 3), f8(edge_scale, n_e)
        fixed = np.ascontiguousarray(fixed, np.uint8).reshape(n_v)
        edge_ij = np.ascontiguousarray(edge_ij, np.int32).reshape(n_e, 2)
        lm_ref, lm_pos = np.ascontiguousarray(lm_ref, np.int32).reshape(n_l), f8(lm_pos, n_l, 3)
        self._reserve(n_v, n_e, n_l)
        o_rot, o_trans, o_scale = np.zeros((n_v, 3, 3)), np.zeros((n_v, 3)), np.zeros(n_v)
        o_lm, info = np.zeros((n_l, 3)), np.zeros(8)
        fs = self._fix_scale if fix_scale is None else bool(fix_scale)
        _lib.check(_lib.lib().ovs_posegraph_optimize(
            self._h, n_v, _ptr(rot), _ptr(trans), _ptr(scale), _ptr(fixed), _ptr(nc_rot), _ptr(nc_trans), _ptr(nc_scale), n_e, _ptr(edge_ij),
            _ptr(edge_rot), _ptr(edge_trans), _ptr(edge_scale), int(fs), int(num_iter), int(pcg_max_iter), n_l, _ptr(lm_ref), _ptr(lm_pos),
            _ptr(o_rot), _ptr(o_trans), _ptr(o_scale), _ptr(o_lm), _ptr(info)), "ovs_posegraph_optimize")
        return o_rot, o_trans, o_scale, o_lm, info

    def optimize(self, problem, num_iter=50, pcg_max_iter=0):
        """problem: io.pose_graph_problem's dict. Returns (poses, landmarks, info): keyframe id -> (rot_cw (3, 3), trans_cw (3)) with upstream's
        write-back rot_cw = R, trans_cw = t / s; landmark id -> pos_w (3); the call's out_info."""
        q = problem
        R, t, s, lm, info = self.optimize_arrays(q["rot"], q["trans"], q["scale"], q["fixed"], q["nc_rot"], q["nc_trans"], q["nc_scale"], q["edge_ij"],
                                                 q["edge_rot"], q["edge_trans"], q["edge_scale"], q["lm_ref"], q["lm_pos"], num_iter, pcg_max_iter)
        poses = {int(k): (R[i].copy(), np.array([t[i, 0] / s[i], t[i, 1] / s[i], t[i, 2] / s[i]])) for i, k in enumerate(q["keyfrm_ids"])}
        return poses, {int(l): lm[i].copy() for i, l in enumerate(q["lm_ids"])}, info
