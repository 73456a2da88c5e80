"""Map database files ("wire / on-disk formats"): read and write the MessagePack map that OpenVSLAM's
`io::map_database_io::save_message_pack / load_message_pack` exchange (expected: src/openvslam/io/map_database_io.cc,
data/map_database.cc `to_json / from_json`, data/keyframe.cc `to_json`, data/landmark.cc `to_json`, data/common.cc
`convert_*_to_json`), and flatten a loaded map into the arrays the device entry points take.

The reference source is absent, so the layout below is restated from the published format -- a `nlohmann::json` object
serialised with `json::to_msgpack` -- as recalled (confidence M; every key is listed here so that a maintainer can diff it against a real
`map.msg` in one look):

  {"cameras":   {name: {"model_type", "setup_type", "color_order", "cols", "rows", "fps", "fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2",
                        "k3", "focal_x_baseline"}},
   "frame_next_id", "keyframe_next_id", "landmark_next_id",
   "keyframes": {"<id>": {"src_frm_id", "ts", "cam", "depth_thr", "rot_cw": [x, y, z, w], "trans_cw": [x, y, z], "n_keypts",
                          "keypts": [{"pt": [x, y], "ang", "oct"}], "undists": [[x, y]], "x_rights": [..], "depths": [..],
                          "descs": [[8 x uint32 = the 32 descriptor bytes, little endian]], "lm_ids": [landmark id or -1],
                          "n_scale_levels", "scale_factor", "span_parent", "span_children": [..], "loop_edges": [..]}},
   "landmarks": {"<id>": {"1st_keyfrm", "pos_w": [x, y, z], "ref_keyfrm", "n_vis", "n_fnd"}}}

Observations are not stored: upstream rebuilds them from the keyframes' `lm_ids` when it loads a map, and so does `map_database`
below. This module is host-side plumbing (no device code); `local_ba_problem` feeds `openvslam_amd.ba.local_ba_optimize`."""
from dataclasses import dataclass, field

import msgpack
import numpy as np

from .ba import EDGE_DTYPE, EDGE_STEREO_DTYPE, quat_to_rot
from .match import KP_DTYPE


@dataclass
class keyframe:
    id: int
    src_frm_id: int = 0
    ts: float = 0.0
    cam: str = "cam"
    depth_thr: float = 0.0
    rot_cw: np.ndarray = None        # quaternion (x, y, z, w), world -> camera
    trans_cw: np.ndarray = None
    keypts: np.ndarray = None        # KP_DTYPE (pt, angle, octave are stored; size / response / class_id are not)
    undists: np.ndarray = None       # (n, 2) float32
    x_rights: np.ndarray = None      # (n,) float32, < 0 = none
    depths: np.ndarray = None
    descs: np.ndarray = None         # (n, 32) uint8
    lm_ids: np.ndarray = None        # (n,) int64, -1 = none
    n_scale_levels: int = 8
    scale_factor: float = 1.2
    span_parent: int = -1
    span_children: list = field(default_factory=list)
    loop_edges: list = field(default_factory=list)
    # not stored in the file: what optimize::global_bundle_adjuster reads and, for a lead keyframe other than 0, writes
    will_be_erased: bool = False
    loop_BA_identifier: int = 0
    rot_cw_after_loop_BA: np.ndarray = None      # cam_pose_cw_after_loop_BA_: quaternion and translation
    trans_cw_after_loop_BA: np.ndarray = None


@dataclass
class landmark:
    id: int
    first_keyfrm: int
    pos_w: np.ndarray
    ref_keyfrm: int
    n_vis: int = 1
    n_fnd: int = 1
    # not stored in the file: openvslam_amd.landmarks.landmark_updater.update_map computes them from the observations
    descriptor: np.ndarray = None      # (32,) uint8
    mean_normal: np.ndarray = None     # (3,) float64
    min_valid_dist: float = None       # the raw members, before the getters' 0.7 / 1.3
    max_valid_dist: float = None
    will_be_erased: bool = False
    loop_BA_identifier: int = 0
    pos_w_after_global_BA: np.ndarray = None


class map_database:
    """data::map_database as far as the hot path needs it: cameras, keyframes, landmarks and the observations derived from lm_ids."""

    def __init__(self):
        self.cameras = {}
        self.keyframes = {}
        self.landmarks = {}
        self.frame_next_id = self.keyframe_next_id = self.landmark_next_id = 0

    def observations(self):
        """landmark id -> [(keyframe id, keypoint index)], keyframes in ascending id (upstream registers them while loading)."""
        obs = {i: [] for i in self.landmarks}
        for kid in sorted(self.keyframes):
            kf = self.keyframes[kid]
            for idx in np.nonzero(kf.lm_ids >= 0)[0]:
                lid = int(kf.lm_ids[idx])
                if lid in obs:
                    obs[lid].append((kid, int(idx)))
        return obs

    def covisibility_weights(self, keyfrm_id):
        """keyframe id -> the number of landmarks it shares with keyfrm_id (graph_node's connected_keyfrms_and_weights_), zeros left out."""
        mine = self.keyframes[keyfrm_id].lm_ids
        mine = set(int(v) for v in mine[mine >= 0])
        w = {}
        for kid, kf in self.keyframes.items():
            if kid == keyfrm_id:
                continue
            ids = kf.lm_ids[kf.lm_ids >= 0]
            n = sum(1 for v in ids if int(v) in mine)
            if n:
                w[kid] = n
        return w

    def covisibilities(self, keyfrm_id, weight_thr=15):
        """graph_node::update_connections: keyframes sharing >= weight_thr landmarks with keyfrm_id (the best one if none reaches it),
        strongest first; ties by ascending id."""
        w = self.covisibility_weights(keyfrm_id)
        keep = [k for k, n in w.items() if n >= weight_thr]
        if not keep and w:
            keep = [max(sorted(w), key=lambda k: w[k])]
        return sorted(keep, key=lambda k: (-w[k], k))


def _descs_to_json(descs):
    return np.ascontiguousarray(descs, np.uint8).reshape(-1, 32).view("<u4").tolist()


def _descs_from_json(rows):
    a = np.asarray(rows, dtype="<u4").reshape(-1, 8)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, 32).copy()


def save_map_database(path, db):
    kfs = {}
    for kid, kf in db.keyframes.items():
        n = len(kf.keypts)
        kfs[str(kid)] = {
            "src_frm_id": int(kf.src_frm_id), "ts": float(kf.ts), "cam": kf.cam, "depth_thr": float(kf.depth_thr),
            "rot_cw": [float(v) for v in kf.rot_cw], "trans_cw": [float(v) for v in kf.trans_cw], "n_keypts": n,
            "keypts": [{"pt": [float(k["x"]), float(k["y"])], "ang": float(k["angle"]), "oct": int(k["octave"])} for k in kf.keypts],
            "undists": [[float(p[0]), float(p[1])] for p in kf.undists], "x_rights": [float(v) for v in kf.x_rights],
            "depths": [float(v) for v in kf.depths], "descs": _descs_to_json(kf.descs), "lm_ids": [int(v) for v in kf.lm_ids],
            "n_scale_levels": int(kf.n_scale_levels), "scale_factor": float(kf.scale_factor), "span_parent": int(kf.span_parent),
            "span_children": [int(v) for v in kf.span_children], "loop_edges": [int(v) for v in kf.loop_edges]}
    lms = {str(lid): {"1st_keyfrm": int(lm.first_keyfrm), "pos_w": [float(v) for v in lm.pos_w], "ref_keyfrm": int(lm.ref_keyfrm),
                      "n_vis": int(lm.n_vis), "n_fnd": int(lm.n_fnd)} for lid, lm in db.landmarks.items()}
    obj = {"cameras": db.cameras, "frame_next_id": int(db.frame_next_id), "keyframe_next_id": int(db.keyframe_next_id),
           "landmark_next_id": int(db.landmark_next_id), "keyframes": kfs, "landmarks": lms}
    with open(path, "wb") as f:
        f.write(msgpack.packb(obj, use_single_float=False))


def load_map_database(path):
    with open(path, "rb") as f:
        obj = msgpack.unpackb(f.read(), raw=False, strict_map_key=False)
    for key in ("cameras", "keyframes", "landmarks"):
        if key not in obj:
            raise ValueError("not an OpenVSLAM map database: key %r missing" % key)
    db = map_database()
    db.cameras = obj["cameras"]
    db.frame_next_id = int(obj.get("frame_next_id", 0))
    db.keyframe_next_id = int(obj.get("keyframe_next_id", 0))
    db.landmark_next_id = int(obj.get("landmark_next_id", 0))
    for sid, j in obj["keyframes"].items():
        n = int(j["n_keypts"])
        kp = np.zeros(n, KP_DTYPE)
        kp["class_id"] = -1
        if n:
            kp["x"] = [k["pt"][0] for k in j["keypts"]]
            kp["y"] = [k["pt"][1] for k in j["keypts"]]
            kp["angle"] = [k["ang"] for k in j["keypts"]]
            kp["octave"] = [k["oct"] for k in j["keypts"]]
        lists = {k: len(j[k]) for k in ("keypts", "undists", "x_rights", "depths", "descs", "lm_ids")}
        if any(v != n for v in lists.values()):
            raise ValueError("keyframe %s: per-keypoint arrays disagree with n_keypts = %d: %s" % (sid, n, lists))
        db.keyframes[int(sid)] = keyframe(
            id=int(sid), src_frm_id=int(j.get("src_frm_id", 0)), ts=float(j.get("ts", 0.0)), cam=j.get("cam", ""), depth_thr=float(j.get("depth_thr", 0.0)),
            rot_cw=np.asarray(j["rot_cw"], np.float64), trans_cw=np.asarray(j["trans_cw"], np.float64), keypts=kp,
            undists=np.asarray(j["undists"], np.float32).reshape(-1, 2), x_rights=np.asarray(j["x_rights"], np.float32),
            depths=np.asarray(j["depths"], np.float32), descs=_descs_from_json(j["descs"]) if n else np.zeros((0, 32), np.uint8),
            lm_ids=np.asarray(j["lm_ids"], np.int64), n_scale_levels=int(j.get("n_scale_levels", 8)), scale_factor=float(j.get("scale_factor", 1.2)),
            span_parent=int(j.get("span_parent", -1)), span_children=list(j.get("span_children", [])), loop_edges=list(j.get("loop_edges", [])))
    for sid, j in obj["landmarks"].items():
        db.landmarks[int(sid)] = landmark(id=int(sid), first_keyfrm=int(j["1st_keyfrm"]), pos_w=np.asarray(j["pos_w"], np.float64),
                                          ref_keyfrm=int(j["ref_keyfrm"]), n_vis=int(j.get("n_vis", 1)), n_fnd=int(j.get("n_fnd", 1)))
    return db


def inv_level_sigma_sq(scale_factor, n_levels):
    """orb_params tables: scale_factors_[l] = scale_factor * scale_factors_[l - 1] in float, level_sigma_sq = sf^2, inverse in float."""
    sf = np.float32(1.0)
    out = []
    for _ in range(int(n_levels)):
        out.append(float(np.float32(1.0) / np.float32(sf * sf)))
        sf = np.float32(scale_factor) * sf
    return np.array(out, np.float64)


def local_ba_problem(db, curr_keyfrm_id):
    """The graph optimize::local_bundle_adjuster::optimize(curr_keyfrm) builds (expected: src/openvslam/optimize/local_bundle_adjuster.cc):
    local keyframes = the current one and its covisibilities; local landmarks = everything they observe; fixed keyframes = the other
    observers of those landmarks; keyframe 0 is fixed too. Returns a dict with the arrays of ovs_local_ba_optimize plus the id lists
    that map rows back to the map (`keyfrm_ids`, `lm_ids`)."""
    kf0 = db.keyframes[curr_keyfrm_id]
    cam = db.cameras[kf0.cam]
    local = [curr_keyfrm_id] + [k for k in db.covisibilities(curr_keyfrm_id) if k != curr_keyfrm_id]
    local_set = set(local)
    obs = db.observations()
    lm_ids = []
    seen = set()
    for kid in local:
        for lid in db.keyframes[kid].lm_ids:
            lid = int(lid)
            if lid >= 0 and lid in db.landmarks and lid not in seen:
                seen.add(lid)
                lm_ids.append(lid)
    fixed = []
    fixed_set = set()
    for lid in lm_ids:
        for kid, _ in obs[lid]:
            if kid not in local_set and kid not in fixed_set:
                fixed_set.add(kid)
                fixed.append(kid)
    keyfrm_ids = local + fixed
    pose_index = {k: i for i, k in enumerate(keyfrm_ids)}
    poses = np.zeros((len(keyfrm_ids), 7))
    for i, k in enumerate(keyfrm_ids):
        kf = db.keyframes[k]
        poses[i, :3] = kf.trans_cw
        poses[i, 3:] = kf.rot_cw
    pose_fixed = np.array([1 if (k in fixed_set or k == 0) else 0 for k in keyfrm_ids], np.uint8)
    points = np.array([db.landmarks[l].pos_w for l in lm_ids], np.float64).reshape(-1, 3)
    mono, stereo = [], []
    inv_sig = {k: inv_level_sigma_sq(db.keyframes[k].scale_factor, db.keyframes[k].n_scale_levels) for k in keyfrm_ids}
    for pi, lid in enumerate(lm_ids):
        for kid, idx in obs[lid]:
            if kid not in pose_index:
                continue
            kf = db.keyframes[kid]
            inv_sigma_sq = float(inv_sig[kid][int(kf.keypts["octave"][idx])])   # inv_level_sigma_sq_[octave]
            ux, uy = float(kf.undists[idx, 0]), float(kf.undists[idx, 1])
            xr = float(kf.x_rights[idx])
            if xr < 0:
                mono.append((pose_index[kid], pi, ux, uy, inv_sigma_sq))
            else:
                stereo.append((pose_index[kid], pi, ux, uy, xr, inv_sigma_sq))
    e_mono = np.zeros(len(mono), EDGE_DTYPE)
    for i, (a, b, x, y, w) in enumerate(mono):
        e_mono[i] = (a, b, x, y, w)
    e_st = np.zeros(len(stereo), EDGE_STEREO_DTYPE)
    for i, (a, b, x, y, r, w) in enumerate(stereo):
        e_st["pose_idx"][i], e_st["point_idx"][i], e_st["obs_x"][i], e_st["obs_y"][i], e_st["obs_x_right"][i], e_st["inv_sigma_sq"][i] = a, b, x, y, r, w
    return {"poses": poses, "pose_fixed": pose_fixed, "points": points, "mono": e_mono, "stereo": e_st,
            "cam": np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float64), "focal_x_baseline": float(cam.get("focal_x_baseline", 0.0)),
            "setup_type": {"Monocular": 0, "Stereo": 1, "RGBD": 2}.get(cam.get("setup_type", "Monocular"), 0),
            "keyfrm_ids": keyfrm_ids, "lm_ids": lm_ids, "n_local": len(local)}


def global_ba_problem(db):
    """The graph optimize::global_bundle_adjuster::optimize builds (expected: src/openvslam/optimize/global_bundle_adjuster.cc): every
    keyframe that is not to be erased, in ascending id, keyframe 0 fixed; every landmark that is not to be erased and has at least one
    observation in such a keyframe (upstream removes a landmark vertex without edges again and does not write it back), in ascending id;
    the edges in upstream's insertion order: landmark by landmark, its observations in the order map_database.observations() gives.
    Returns the arrays of ovs_global_ba_optimize plus `keyfrm_ids` and `lm_ids`, which map rows back to the map, `model` (0 perspective,
    1 equirectangular) and `cols` / `rows`."""
    keyfrm_ids = [k for k in sorted(db.keyframes) if not db.keyframes[k].will_be_erased]
    pose_index = {k: i for i, k in enumerate(keyfrm_ids)}
    cam = db.cameras[db.keyframes[keyfrm_ids[0]].cam] if keyfrm_ids else {}
    equirect = cam.get("model_type") == "Equirectangular"
    obs = db.observations()
    inv_sig = {k: inv_level_sigma_sq(db.keyframes[k].scale_factor, db.keyframes[k].n_scale_levels) for k in keyfrm_ids}
    lm_ids, mono, stereo = [], [], []
    for lid in sorted(db.landmarks):
        if db.landmarks[lid].will_be_erased:
            continue
        seen = [(kid, idx) for kid, idx in obs[lid] if kid in pose_index]
        if not seen:
            continue
        pi = len(lm_ids)
        lm_ids.append(lid)
        for kid, idx in seen:
            kf = db.keyframes[kid]
            w = float(inv_sig[kid][int(kf.keypts["octave"][idx])])
            ux, uy, xr = float(kf.undists[idx, 0]), float(kf.undists[idx, 1]), float(kf.x_rights[idx])
            if xr < 0 or equirect:
                mono.append((pose_index[kid], pi, ux, uy, w))
            else:
                stereo.append((pose_index[kid], pi, ux, uy, xr, w))
    poses = np.zeros((len(keyfrm_ids), 7))
    for i, k in enumerate(keyfrm_ids):
        poses[i, :3] = db.keyframes[k].trans_cw
        poses[i, 3:] = db.keyframes[k].rot_cw
    e_mono = np.array(mono, EDGE_DTYPE) if mono else np.zeros(0, EDGE_DTYPE)
    e_st = np.array(stereo, EDGE_STEREO_DTYPE) if stereo else np.zeros(0, EDGE_STEREO_DTYPE)
    return {"poses": poses, "pose_fixed": np.array([1 if k == 0 else 0 for k in keyfrm_ids], np.uint8),
            "points": np.array([db.landmarks[l].pos_w for l in lm_ids], np.float64).reshape(-1, 3), "mono": e_mono, "stereo": e_st,
            "cam": np.array([cam.get("fx", 0.0), cam.get("fy", 0.0), cam.get("cx", 0.0), cam.get("cy", 0.0)], np.float64),
            "focal_x_baseline": float(cam.get("focal_x_baseline", 0.0)),
            "setup_type": {"Monocular": 0, "Stereo": 1, "RGBD": 2}.get(cam.get("setup_type", "Monocular"), 0),
            "model": 1 if equirect else 0, "cols": int(cam.get("cols", 0)), "rows": int(cam.get("rows", 0)),
            "keyfrm_ids": keyfrm_ids, "lm_ids": lm_ids}


def _sim3(R, t, s):
    return [float(v) for v in np.asarray(R, np.float64).ravel()], [float(v) for v in np.asarray(t, np.float64).ravel()], float(s)


def _sim3_inverse(S):
    """DESIGN.md 3.19 rule G1 in Python floats: R' = R^T, s' = 1 / s, t' = (-s') (R^T t)."""
    R, t, s = S
    si = 1.0 / s
    return ([R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]],
            [(-si) * ((R[r] * t[0] + R[3 + r] * t[1]) + R[6 + r] * t[2]) for r in range(3)], si)


def _sim3_product(A, B):
    """Rule G1's A B = (R_A R_B, s_A (R_A t_B) + t_A, s_A s_B), every sum left to right."""
    Ra, ta, sa = A
    Rb, tb, sb = B
    return ([(Ra[3 * i] * Rb[j] + Ra[3 * i + 1] * Rb[3 + j]) + Ra[3 * i + 2] * Rb[6 + j] for i in range(3) for j in range(3)],
            [sa * ((Ra[3 * i] * tb[0] + Ra[3 * i + 1] * tb[1]) + Ra[3 * i + 2] * tb[2]) + ta[i] for i in range(3)], sa * sb)


def pose_graph_problem(db, loop_keyfrm_id, curr_keyfrm_id, non_corrected, pre_corrected, loop_connections, min_weight=100):
    """The graph optimize::graph_optimizer::optimize(loop_keyfrm, curr_keyfrm, non_corrected_Sim3s, pre_corrected_Sim3s, loop_connections)
    builds (expected: src/openvslam/optimize/graph_optimizer.cc, as recalled), as the flat arrays of ovs_posegraph_optimize.
    non_corrected / pre_corrected: keyframe id -> (R (3, 3), t (3), s), the Sim3_cw before / after the loop's correction of the current
    keyframe's neighbourhood; loop_connections: keyframe id -> the ids it newly connects to. Vertices in ascending keyframe id: a vertex
    starts from pre_corrected if present, otherwise from (rot_cw, trans_cw, 1.0); the loop keyframe is fixed. Edges, measurement Sim3_21 =
    Sim3_2w Sim3_1w^-1 with vertex 0 = keyframe 1, in upstream's order: (a) the loop connections from the vertices' start states, kept at
    weight >= min_weight or when the pair is (current, loop); then per keyframe in ascending id, with the non-corrected Sim3 of either end
    where there is one: (b) its spanning-tree parent, (c) its earlier loop edges (id2 < id1), (d) its covisibilities of weight >= min_weight
    that are neither its parent nor its child nor a loop edge, id2 < id1, and whose pair has not been inserted by (a). The landmark
    write-back reads the start state of the landmark's reference keyframe (upstream's Sim3s_cw), so nc_* are the start states. Returns the
    arrays plus keyfrm_ids, lm_ids and edge_class (one of "loop", "parent", "loop_edge", "covis" per edge)."""
    keyfrm_ids = sorted(db.keyframes)
    index = {k: i for i, k in enumerate(keyfrm_ids)}
    start = {}
    for k in keyfrm_ids:
        kf = db.keyframes[k]
        start[k] = _sim3(*pre_corrected[k]) if k in pre_corrected else _sim3(quat_to_rot(kf.rot_cw), kf.trans_cw, 1.0)
    nc = {k: _sim3(*v) for k, v in non_corrected.items()}
    edges, meas, classes, inserted = [], [], [], set()

    def insert(id1, id2, S_1w, S_2w, cls):
        edges.append((index[id1], index[id2]))
        meas.append(_sim3_product(S_2w, _sim3_inverse(S_1w)))
        classes.append(cls)

    for id1 in sorted(loop_connections):   # (upstream walks a map and sets keyed by pointer, which is no order: ascending ids here)
        w = db.covisibility_weights(id1)
        for id2 in sorted(loop_connections[id1]):
            if (id1 != curr_keyfrm_id or id2 != loop_keyfrm_id) and w.get(id2, 0) < min_weight:
                continue
            insert(id1, id2, start[id1], start[id2], "loop")
            inserted.add((min(id1, id2), max(id1, id2)))
    of = lambda k: nc[k] if k in nc else start[k]
    for id1 in keyfrm_ids:
        kf = db.keyframes[id1]
        parent = kf.span_parent if kf.span_parent in index else -1
        if parent >= 0:
            insert(id1, parent, of(id1), of(parent), "parent")
        for id2 in kf.loop_edges:
            if id2 in index and id2 < id1:
                insert(id1, id2, of(id1), of(id2), "loop_edge")
        w = db.covisibility_weights(id1)
        for id2 in sorted((k for k, n in w.items() if n >= min_weight), key=lambda k: (-w[k], k)):
            if id2 == parent or id2 in kf.span_children or id2 in kf.loop_edges or not id2 < id1:
                continue
            if (id2, id1) in inserted:
                continue
            insert(id1, id2, of(id1), of(id2), "covis")
    lm_ids = sorted(db.landmarks)
    n_v, n_e = len(keyfrm_ids), len(edges)
    S = [start[k] for k in keyfrm_ids]
    arr = lambda rows, w: np.array(rows, np.float64).reshape(len(rows), w)
    return {"rot": arr([s[0] for s in S], 9), "trans": arr([s[1] for s in S], 3), "scale": np.array([s[2] for s in S], np.float64),
            "fixed": np.array([1 if k == loop_keyfrm_id else 0 for k in keyfrm_ids], np.uint8),
            "nc_rot": arr([s[0] for s in S], 9), "nc_trans": arr([s[1] for s in S], 3), "nc_scale": np.array([s[2] for s in S], np.float64),
            "edge_ij": np.array(edges, np.int32).reshape(n_e, 2), "edge_rot": arr([m[0] for m in meas], 9),
            "edge_trans": arr([m[1] for m in meas], 3), "edge_scale": np.array([m[2] for m in meas], np.float64),
            "lm_ref": np.array([index.get(db.landmarks[l].ref_keyfrm, -1) for l in lm_ids], np.int32),
            "lm_pos": arr([[float(v) for v in db.landmarks[l].pos_w] for l in lm_ids], 3), "keyfrm_ids": keyfrm_ids, "lm_ids": lm_ids,
            "edge_class": classes, "n_vertices": n_v}


def top_covisibilities_of(map_db, n=10):
    """graph_node::get_top_n_covisibilities(n) of a loaded map as the callable bow_database.acquire_* take: id -> at most n ids, strongest first."""
    return lambda keyfrm_id: map_db.covisibilities(keyfrm_id)[:n]


def bow_database_of(map_db, vocabulary, levelsup=4, max_words=4096, device=0):
    """data::bow_database filled from a loaded map, as upstream's map loader registers every keyframe (compute_bow from the stored
    descriptors, then bow_db->add_keyframe), in ascending keyframe id. Query it with top_covisibilities_of(map_db)."""
    from .bow import bow_database
    db = bow_database(max(len(map_db.keyframes), 1), max_words=max_words, device=device)
    for kid in sorted(map_db.keyframes):
        db.add_keyframe(kid, vocabulary.transform(map_db.keyframes[kid].descs, levelsup)[0])
    return db
