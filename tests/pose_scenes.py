"""Constructed frames for optimize::pose_optimizer::optimize (ORACLE_SPEC rules 25 / 26): every size at which the host entry changes the
launch form, and every exit of the Levenberg-Marquardt loop that random frames do not reach, built ON PURPOSE. Pure numpy on top of
openvslam_amd.synth.synth_pose_frame / synth_pose_frame_equirect; no GPU, no oracle at import. tests/test_pose_scenes.py asserts on the CPU that
every frame still does what it was built for and that the reference is well defined on it (two independent CPU implementations agree; the
oracle's own spread under permutations of the observations is a quarter of the tolerance the device is held to, and no observation sits on a
chi-square gate); tests/test_gpu_pose.py then holds the HIP kernel to the oracle on the same frames, in every launch form.

A frame is a Frame: name, model ("persp" | "equirect"), the input pose, the observation records, cam = (fx, fy, cx, cy) or (cols, rows), the
focal length x baseline (perspective) and `expect`: the outcome it was built for (checked against the oracle on the CPU).

The launch forms of ovs_pose_optimize, by number of observations n (pose_optimize_host):
    n <  500   1 workgroup            n <= 2 * groups * 256: a thread's (at most two) records live in registers
    n <  850   2 workgroups           ... so the register form ends at 512 / 1024 / 2048 / 4096 observations for 1 / 2 / 4 / 8 workgroups
    n < 1600   4 workgroups           one workgroup of 768 (equirectangular: 1500) or more observations has 512 threads
    n >= 1600  8 workgroups           256-thread workgroups: 256 | 512 | ... are the sizes where a thread's second, third, ... record starts
"""
from typing import NamedTuple

import numpy as np

from openvslam_amd.synth import equirect_project, synth_pose_frame, synth_pose_frame_equirect

POSE_OBS_DTYPE = np.dtype([("pos_w", "<f8", (3,)), ("obs_x", "<f8"), ("obs_y", "<f8"), ("obs_x_right", "<f8"), ("inv_sigma_sq", "<f8"),
                           ("is_stereo", "<i4"), ("pad", "<i4")])
TOL = {"persp": 1e-9, "equirect": 2e-8}       # the pose tolerances of tests/test_gpu_pose.py
GATE_2D, GATE_3D = float(np.float32(5.99146)), float(np.float32(7.81473))


class Frame(NamedTuple):
    name: str
    model: str
    T0: np.ndarray
    obs: np.ndarray
    cam: tuple
    bf: float
    expect: dict


class Row(NamedTuple):
    """One line of edge_frames(): the arguments of the synth_pose_frame* call."""
    model: str
    n: int
    seed: int
    stereo_frac: float = 0.0
    outlier_frac: float = 0.1
    pose_err: float = 1.0
    seam_frac: float = 0.0
    pole_frac: float = 0.0

    @property
    def name(self):
        return ("p%d" if self.model == "persp" else "e%d") % self.n


PERSP_SIZES = (5, 6, 255, 256, 257, 499, 500, 511, 512, 513, 767, 768, 849, 850, 1023, 1024, 1025, 1599, 1600, 2047, 2048, 2049, 4095, 4096, 4097,
               8191, 8192)
EQUIRECT_SIZES = (5, 256, 257, 499, 500, 849, 850, 1499, 1500, 1599, 1600, 4096, 4097, 8192)
EXTRA_SIZES = (63, 300, 2600)       # sizes of the forced-form and batch tests that are not edges of the host's table
# seed = n unless the oracle's own permutation spread on that frame exceeds a quarter of the tolerance, or an observation sits on a chi-square gate
# (tests/test_pose_scenes.py checks both for every row): then the next seed n + 10000 k that passes
_SEED = {("persp", 5): 10005, ("persp", 6): 10006, ("persp", 500): 10500, ("persp", 1024): 21024, ("persp", 2048): 12048,
         ("persp", 2600): 12600, ("persp", 4096): 14096, ("persp", 4097): 24097, ("persp", 8191): 28191, ("persp", 8192): 38192,
         ("equirect", 500): 10500}


def _row(model, n, k):
    seed = _SEED.get((model, n), n)
    of = 0.15 if n == 8192 else 0.1       # (8192: enough outliers that some fall among the last 256 observations, a thread's mask bit 31)
    if model == "persp":
        return Row(model, n, seed, stereo_frac=(0.0, 0.4, 1.0)[k % 3], outlier_frac=of)
    return Row(model, n, seed, outlier_frac=of, seam_frac=0.05, pole_frac=0.05)


def edge_frames():
    """The table of frames at the sizes where the launch form changes: perspective rows with stereo fractions 0, 0.4 and 1 dealt over the rows,
    then the equirectangular subset with a twentieth of the bearings at the seam and a twentieth at the poles."""
    return tuple(_row("persp", n, k) for k, n in enumerate(PERSP_SIZES)) + tuple(_row("equirect", n, k) for k, n in enumerate(EQUIRECT_SIZES))


def extra_frames():
    """Sizes between the edges (forced workgroup counts, batch launches). Perspective: 63 all stereo (shorter than a workgroup, beside the
    mono-only p5 in a batch), 300 and 2600 mixed; the equirectangular ones beside them, and 513."""
    sf = {63: 1.0, 300: 0.4, 2600: 0.4}
    return tuple(Row("persp", n, _SEED.get(("persp", n), n), stereo_frac=sf[n]) for n in EXTRA_SIZES) + \
        tuple(Row("equirect", n, _SEED.get(("equirect", n), n), seam_frac=0.05, pole_frac=0.05) for n in EXTRA_SIZES + (513,))


def row_by_name(name):
    for r in edge_frames() + extra_frames():
        if r.name == name:
            return r
    raise KeyError(name)


def make(row):
    """Row -> Frame."""
    if row.model == "persp":
        T0, obs, cam, bf, _ = synth_pose_frame(POSE_OBS_DTYPE, row.n, row.seed, row.stereo_frac, row.outlier_frac, row.pose_err)
        return Frame(row.name, "persp", T0, obs, cam, bf, {})
    T0, obs, cols, rows, _ = synth_pose_frame_equirect(POSE_OBS_DTYPE, row.n, row.seed, outlier_frac=row.outlier_frac, pose_err=row.pose_err,
                                                       seam_frac=row.seam_frac, pole_frac=row.pole_frac)
    return Frame(row.name, "equirect", T0, obs, (cols, rows), 0.0, {})


# ---- constructed scenes ------------------------------------------------------------------------------------------------------------------
def _project(model, T, obs, cam, bf):
    pc = obs["pos_w"] @ T[:, :3].T + T[:, 3]
    if model == "equirect":
        u, v = equirect_project(pc, cam[0], cam[1])
        return pc, u, v, np.zeros(len(obs))
    u = cam[0] * pc[:, 0] / pc[:, 2] + cam[2]
    return pc, u, cam[1] * pc[:, 1] / pc[:, 2] + cam[3], u - bf / pc[:, 2]


def _base(model, n, seed, stereo_frac=0.0, pose_err=1.0, outlier_frac=0.0):
    if model == "persp":
        T0, obs, cam, bf, (Rt, tt, _) = synth_pose_frame(POSE_OBS_DTYPE, n, seed, stereo_frac, outlier_frac, pose_err)
    else:
        T0, obs, cols, rows, (Rt, tt, _) = synth_pose_frame_equirect(POSE_OBS_DTYPE, n, seed, outlier_frac=outlier_frac, pose_err=pose_err)
        cam, bf = (cols, rows), 0.0
    return T0, obs, cam, bf, np.concatenate([Rt, tt[:, None]], 1)


def perfect(model, n, stereo_frac=0.0):
    """Noise-free observations and T0 = the true pose: the frame is optimal before the first step (residuals of a few ulps of a pixel: the
    rounding of the projection). The estimate may not move by more than an ulp of its entries and nothing is flagged."""
    _, obs, cam, bf, Tt = _base(model, n, 1000 + n, stereo_frac, pose_err=0.0)
    _, u, v, ur = _project(model, Tt, obs, cam, bf)
    obs["obs_x"], obs["obs_y"] = u, v
    obs["obs_x_right"] = np.where(obs["is_stereo"] != 0, ur, 0.0)
    return Frame("perfect_%s%d" % (model[0], n), model, Tt.copy(), obs, cam, bf, dict(nv=n, flagged=0, pose_atol=1e-15))


def zero_weights(model):
    """inv_sigma_sq = 0 for every observation: H = 0, b = 0, so lambda = 1e-5 max diag(H) = 0 and the Cholesky of H + lambda I fails in the first
    trial and in all nine retries (lambda stays 0) -- an iteration with ten failed solves and not one accepted step, in each of the four rounds.
    Every chi-square is 0: nothing is flagged and the pose is the input pose bit for bit."""
    T0, obs, cam, bf, _ = _base(model, 64, 2064, 0.4)
    obs["inv_sigma_sq"] = 0.0
    return Frame("zero_weights_" + model[0], model, T0, obs, cam, bf, dict(nv=64, flagged=0, pose_equal=True))


def few_inliers(model, keep):
    """n = 40, small pose error; the first `keep` (4, 5 or 6) observations are left alone and the others moved by 200 to 400 px. After the first
    round fewer than five observations are inliers, so the loop over the rounds leaves there (upstream: num_init_obs - num_bad_obs < 5)."""
    T0, obs, cam, bf, _ = _base(model, 40, 3040 + keep, 0.4, pose_err=0.2)
    rng = np.random.default_rng(40 + keep)
    m = 40 - keep
    ang = rng.uniform(0, 2 * np.pi, m)
    r = rng.uniform(200, 400, m)
    obs["obs_x"][keep:] += r * np.cos(ang)
    obs["obs_y"][keep:] += r * np.sin(ang)
    return Frame("few_inliers_%s%d" % (model[0], keep), model, T0, obs, cam, bf, dict(nv_below=5, rounds_left_early=True))


def survivors(model, keep):
    """Exactly `keep` (4 or 5) inliers after the FIRST round, so that the test `n - num_bad < 5` decides: few_inliers with the moved observations
    at sigma = 50 px. Their Huber-bounded pull (2 delta sqrt(inv_sigma_sq) each) is then a fiftieth of what the untouched noise-free
    observations at sigma = 1 px answer with for a pixel of displacement, so those stay far inside their gates while every moved one
    (chi-square 16 and more) is flagged. keep = 4: the loop leaves after the first round, with the pose the outliers still pulled on. keep = 5: the three other
    rounds run on five noise-free observations and end at the true pose."""
    T0, obs, cam, bf, Tt = _base(model, 40, 6040 + keep, 0.4, pose_err=0.2)
    _, u, v, ur = _project(model, Tt, obs, cam, bf)
    rng = np.random.default_rng(60 + keep)
    m = 40 - keep
    ang = rng.uniform(0, 2 * np.pi, m)
    r = rng.uniform(200, 400, m)
    obs["obs_x"][:keep], obs["obs_y"][:keep] = u[:keep], v[:keep]
    obs["obs_x_right"][:keep] = np.where(obs["is_stereo"][:keep] != 0, ur[:keep], 0.0)
    obs["inv_sigma_sq"][:keep] = 1.0
    obs["obs_x"][keep:] += r * np.cos(ang)
    obs["obs_y"][keep:] += r * np.sin(ang)
    obs["inv_sigma_sq"][keep:] = 0.0004
    return Frame("survivors_%s%d" % (model[0], keep), model, T0, obs, cam, bf, dict(nv=keep, rounds=1 if keep < 5 else 4))


def behind_camera():
    """n = 300 with the depth of every tenth landmark negated: those project through the camera centre (negative z, mirrored image point) and
    are flagged in the first round together with the frame's gross outliers; the pose stays finite."""
    T0, obs, cam, bf, _ = _base("persp", 300, 4300, 0.4, outlier_frac=0.1)
    obs["pos_w"][::10, 2] *= -1.0
    return Frame("behind_camera", "persp", T0, obs, cam, bf, dict(flagged_idx=np.arange(0, 300, 10), finite=True))


def one_landmark():
    """Twelve copies of one record: twelve times the same two (three) Jacobian rows, so H has rank 2 (3) and only the damping makes it
    positive definite; entry (3, 4) of H is an exact zero (row 0 has no y-translation term, row 1 no x-translation term)."""
    T0, obs, cam, bf, _ = _base("persp", 12, 5012, 1.0)
    obs[:] = obs[0]
    return Frame("one_landmark", "persp", T0, obs, cam, bf, dict(finite=True))


def scenes():
    """Every constructed scene, perspective then the equirectangular twins."""
    out = [perfect("persp", 64), perfect("persp", 600, 0.5), zero_weights("persp")]
    out += [few_inliers("persp", k) for k in (4, 5, 6)]
    out += [behind_camera(), one_landmark(), perfect("equirect", 64), perfect("equirect", 600), zero_weights("equirect")]
    out += [few_inliers("equirect", k) for k in (4, 5, 6)]
    out += [survivors(m, k) for m in ("persp", "equirect") for k in (4, 5)]
    return tuple(out)


def frame_by_name(name):
    for s in scenes():
        if s.name == name:
            return s
    return make(row_by_name(name))


# ---- helpers shared by the CPU and the GPU tests -------------------------------------------------------------------------------------------
def chi2_at(frame, T):
    """(chi-square of every observation at pose T, its gate): numpy, for the distance-to-gate checks (not the oracle's operation order)."""
    _, u, v, ur = _project(frame.model, T, frame.obs, frame.cam, frame.bf)
    st = (frame.obs["is_stereo"] != 0) & (frame.model == "persp")
    e2 = (frame.obs["obs_x"] - u) ** 2 + (frame.obs["obs_y"] - v) ** 2 + np.where(st, (frame.obs["obs_x_right"] - ur) ** 2, 0.0)
    return e2 * frame.obs["inv_sigma_sq"], np.where(st, GATE_3D, GATE_2D)


def run(mod, frame, obs=None):
    """frame through mod.pose_optimize / pose_optimize_equirect (mod: the oracle binding, tests/nversion_pose.py or openvslam_amd.ba)."""
    o = frame.obs if obs is None else obs
    if frame.model == "persp":
        return mod.pose_optimize(frame.T0, o, frame.cam, frame.bf)
    return mod.pose_optimize_equirect(frame.T0, o, frame.cam[0], frame.cam[1])


_REF = {}


def reference(oracle, frame):
    """The oracle's (pose, flags, num_valid) of a frame, computed once per process and shared (callers must not modify it)."""
    if frame.name not in _REF:
        T, out, nv = run(oracle, frame)
        T.setflags(write=False)
        out.setflags(write=False)
        _REF[frame.name] = (T, out, int(nv))
    return _REF[frame.name]


def pack(T, out, nv):
    """One result as a flat float array (what the child processes of the forced-form tests store per frame)."""
    return np.concatenate([np.asarray(T, float).ravel(), np.asarray(out).astype(float), [float(nv)]])


def unpack(a):
    return a[:12].reshape(3, 4), a[12:-1] != 0, int(a[-1])
