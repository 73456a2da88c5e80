"""The batch solvers' host plan (openvslam_amd/csrc/solve_plan.inc) without a device: tests/solve_plan_host.cc, built by the plain host compiler
from the plan alone, answers the rows below on stdin. The expected values are written out by hand from the code as it stood before the plan was moved
out of the nine units (each unit's layout_of, the head of run_staged and run_batch, each extern "C" body's first lines and its stage / collect
lambdas), not generated from the plan. The GPU tests see results and statuses only; where a byte of a staged block lands is visible here."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
EXE = os.path.join(CPP, "solve_plan_host")
OK, INVALID, CAPACITY = 0, -1, -4
SIZES = [(1, 0), (1, 1), (1, 2), (2, 3), (3, 70), (65535, 1), (1, 1 << 20)]


def even(x):
    return (x + 1) & ~1


def al16(x):
    return (x + 15) & ~15


# ---- layouts: family -> (P, T) -> [(section, offset, bytes, alignment of its element)], in the Layout's order; then the names of what follows them
def lay_sim3(P, T):
    cams = 8 * P
    p1 = cams + 40 * 2 * P
    thr1 = p1 + 48 * T
    off = thr1 + 8 * even(T)
    return [("keys", 0, 8 * P, 8), ("cams", cams, 80 * P, 8), ("p1", p1, 24 * T, 8), ("p2", p1 + 24 * T, 24 * T, 8), ("thr1", thr1, 4 * T, 4),
            ("thr2", thr1 + 4 * even(T), 4 * T, 4), ("offsets", off, 4 * (P + 1), 4)], [off + 4 * (P + 1)]


def lay_pnp(P, T):
    off = 8 * P + 56 * T
    return [("keys", 0, 8 * P, 8), ("bearings", 8 * P, 24 * T, 8), ("pos_w", 8 * P + 24 * T, 24 * T, 8), ("max_cos", 8 * P + 48 * T, 8 * T, 8),
            ("offsets", off, 4 * (P + 1), 4)], [off + 4 * (P + 1)]


def lay_sim3opt(P, T):
    p1 = 80 * P + 104 * P
    w1 = p1 + 80 * T
    off = w1 + 8 * even(T)
    work = off + 4 * (P + 1)
    return [("cams", 0, 80 * P, 8), ("init", 80 * P, 104 * P, 8), ("p1", p1, 24 * T, 8), ("p2", p1 + 24 * T, 24 * T, 8), ("obs1", p1 + 48 * T, 16 * T, 8),
            ("obs2", p1 + 64 * T, 16 * T, 8), ("w1", w1, 4 * T, 4), ("w2", w1 + 4 * even(T), 4 * T, 4), ("offsets", off, 4 * (P + 1), 4),
            ("work", work, T, 1)], [work + T]


def lay_twoview(P, T):
    return [("x1", 0, 16 * T, 8), ("x2", 16 * T, 16 * T, 8), ("offsets", 32 * T, 4 * (P + 1), 4)], [32 * T + 4 * (P + 1)]


def lay_essential(P, T):
    return [("b1", 0, 24 * T, 8), ("b2", 24 * T, 24 * T, 8), ("offsets", 48 * T, 4 * (P + 1), 4)], [48 * T + 4 * (P + 1)]


def lay_reconstruct(P, T):
    kp1 = 112 * P
    off = kp1 + 80 * T
    inl = off + 4 * (P + 1)
    return [("problems", 0, 112 * P, 8), ("kp1", kp1, 16 * T, 8), ("kp2", kp1 + 16 * T, 16 * T, 8), ("b1", kp1 + 32 * T, 24 * T, 8),
            ("b2", kp1 + 56 * T, 24 * T, 8), ("offsets", off, 4 * (P + 1), 4), ("inlier", inl, T, 1)], [inl + T]


def lay_triangulate(P, T):
    Te = even(T)
    f32 = 352 * P + 48 * T
    pidx = f32 + 48 * Te
    off = pidx + 4 * Te
    pos = off + 4 * even(P + 1)
    return [("problems", 0, 352 * P, 8), ("b1", 352 * P, 24 * T, 8), ("b2", 352 * P + 24 * T, 24 * T, 8), ("f32", f32, 48 * Te, 4), ("pidx", pidx, 4 * T, 4),
            ("offsets", off, 4 * (P + 1), 4), ("pos", pos, 24 * T, 8), ("status", pos + 24 * T, T, 1), ("method", pos + 25 * T, T, 1)], [pos + 26 * T, Te]


def lay_landmarks(P, T, with_desc):
    p4, t4 = al16(4 * P), al16(4 * T)
    sf = al16(24 * P)
    off = sf + 2 * p4
    slot = off + al16(4 * (P + 1))
    n_used = slot + 2 * t4
    kp = n_used + 3 * p4
    desc = kp + t4
    normal = desc + 32 * T
    rng = normal + al16(24 * P)
    best = rng + al16(8 * P)
    total = best + p4 + 32 * P
    return [("pos", 0, 24 * P, 16), ("sf_ref", sf, 4 * P, 16), ("ref_slot", sf + p4, 4 * P, 16), ("offsets", off, 4 * (P + 1), 16), ("obs_slot", slot, 4 * T, 16),
            ("used", slot + t4, 4 * T, 16), ("n_used", n_used, 4 * P, 16), ("list8", n_used + p4, 4 * P, 16), ("list64", n_used + 2 * p4, 4 * P, 16),
            ("obs_kp", kp, 4 * T, 16), ("desc", desc, 32 * T, 16), ("normal", normal, 24 * P, 16), ("range", rng, 8 * P, 16), ("best", best, 4 * P, 16),
            ("out_desc", best + p4, 32 * P, 16)], [total, normal if with_desc else desc]


LAYOUTS = {"sim3": lay_sim3, "pnp": lay_pnp, "sim3opt": lay_sim3opt, "twoview": lay_twoview, "essential": lay_essential, "reconstruct": lay_reconstruct,
           "triangulate": lay_triangulate, "landmarks:desc=0": lambda P, T: lay_landmarks(P, T, False), "landmarks:desc=1": lambda P, T: lay_landmarks(P, T, True)}


def layout_row(key, P, T):
    fam, _, extra = key.partition(":")
    return "layout:%s:P=%d:T=%d%s" % (fam, P, T, ":" + extra if extra else "")


# ---- error contracts: family -> (what every row starts from, [(keys, status)]); the rows of the family's test_error_contract in tests/test_gpu_*.py,
# the precedence rows and P = 0. A status alone stands for (status, 0, 0): refused, nothing to run.
def ok(T):
    return (OK, T, 1)


NOTHING = (OK, 0, 0)   # no problems: OK, and nothing runs
RANSAC_ROWS = [("max_num_iter=0", INVALID), ("max_num_iter=1048577", INVALID), ("P=3:off=0,20,40,60", CAPACITY), ("off=0,71", CAPACITY), ("P=0:off=0", NOTHING),
               ("P=0:off=0:max_num_iter=0", INVALID), ("P=0:off=0:h=0", INVALID), ("P=0:off=-:null=out_valid", NOTHING), ("max_num_iter=1048576:off=0,3", ok(3))]
HEAD_ROWS = [("", ok(65)), ("h=0", INVALID), ("off=-", INVALID), ("P=-1:off=-", INVALID), ("P=-1", INVALID), ("off=1,65", INVALID), ("P=2:off=0,40,30", INVALID),
             ("off=0,70", ok(70)), ("P=2:off=0,35,70", ok(70))]
CONTRACTS = {
    "sim3": ("", HEAD_ROWS + RANSAC_ROWS + [
        ("null=p1", INVALID), ("null=thr1", INVALID), ("null=cams_1", INVALID), ("null=out_valid", INVALID), ("null=out_flags", INVALID), ("null=out_scale", INVALID),
        ("min_num_inliers=-1", INVALID), ("cam1=model2", INVALID), ("cam1=nanfx", INVALID), ("cam1=infcy", INVALID), ("cam1=norows", INVALID),
        ("cam2=model2", INVALID), ("P=2:off=0,2,2", ok(2)), ("P=2:off=0,0,0:null=p1+p2+thr1+thr2+out_flags", ok(0)),
        ("P=3:off=0,20,40,60:cam1=model2", CAPACITY), ("off=0,71:cam2=norows", CAPACITY), ("P=0:off=0:min_num_inliers=-1", INVALID)]),
    "pnp": ("", HEAD_ROWS + RANSAC_ROWS + [
        ("null=bearings", INVALID), ("null=pos_w", INVALID), ("null=max_cos_errors", INVALID), ("null=out_valid", INVALID), ("null=out_rot", INVALID),
        ("null=out_flags", INVALID), ("min_num_inliers=-1", INVALID), ("P=2:off=0,3,3", ok(3))]),
    "sim3opt": ("", HEAD_ROWS + [
        ("null=p1", INVALID), ("null=obs1", INVALID), ("null=inv_sigma_sq_1", INVALID), ("null=cams_1", INVALID), ("null=rot_12_in", INVALID),
        ("null=out_num_inliers", INVALID), ("null=out_flags", INVALID), ("num_iter=0", INVALID), ("chi_sq=0", INVALID), ("chi_sq=nan", INVALID),
        ("chi_sq=inf", INVALID), ("cam1=model2", INVALID), ("cam1=nanfx", INVALID), ("cam1=norows", INVALID), ("P=3:off=0,20,40,60", CAPACITY),
        ("off=0,71", CAPACITY), ("P=0:off=0", NOTHING), ("P=2:off=0,0,0", ok(0)), ("P=3:off=0,20,40,60:cam1=norows", CAPACITY),
        ("P=0:off=0:chi_sq=0", INVALID), ("P=0:off=0:num_iter=0", INVALID), ("h=0:P=0:off=0", INVALID)]),
    "twoview": ("", HEAD_ROWS + [
        ("null=x1", INVALID), ("null=x2", INVALID), ("null=out_H_21", INVALID), ("null=out_valid", INVALID), ("null=out_selected", INVALID),
        ("null=out_flags_H", INVALID), ("null=out_flags_F", INVALID), ("max_num_iter=0", INVALID), ("max_num_iter=1048577", INVALID), ("models=0", INVALID),
        ("models=4", INVALID), ("sigma=0", INVALID), ("sigma=nan", INVALID), ("sigma=inf", INVALID), ("P=3:off=0,20,40,60", CAPACITY), ("off=0,71", CAPACITY),
        ("P=0:off=0", NOTHING), ("P=2:off=0,7,7", ok(7)), ("P=0:off=0:models=0", INVALID), ("P=0:off=0:sigma=0", INVALID)]),
    "essential": ("", HEAD_ROWS + [
        ("null=bearings_1", INVALID), ("null=bearings_2", INVALID), ("null=out_E_21", INVALID), ("null=out_scores", INVALID), ("null=out_valid", INVALID),
        ("null=out_best_iter", INVALID), ("null=out_num_inliers", INVALID), ("null=out_flags", INVALID), ("max_num_iter=0", INVALID),
        ("max_num_iter=1048577", INVALID), ("residual_cos_thr=0", INVALID), ("residual_cos_thr=-0.01", INVALID), ("residual_cos_thr=1.0000001", INVALID),
        ("residual_cos_thr=nan", INVALID), ("residual_cos_thr=inf", INVALID), ("residual_cos_thr=1.0", ok(65)), ("P=3:off=0,20,40,60", CAPACITY),
        ("off=0,71", CAPACITY), ("P=0:off=0", NOTHING), ("P=2:off=0,7,7", ok(7)), ("P=0:off=0:residual_cos_thr=0", INVALID)]),
    "reconstruct": ("maxt=100:off=0,81", [
        ("", ok(81)), ("h=0", INVALID), ("off=-", INVALID), ("null=models", INVALID), ("null=mats", INVALID), ("null=cams", INVALID), ("null=inlier_flags", INVALID),
        ("null=keypts_ref", INVALID), ("null=bearings_cur", INVALID), ("null=out_success", INVALID), ("null=out_rot", INVALID),
        ("null=out_triangulated_pts", INVALID), ("null=out_is_triangulated", INVALID), ("P=-1", INVALID), ("off=1,81", INVALID),
        ("P=2:off=0,40,30", INVALID), ("models=0", INVALID), ("models=3", INVALID), ("reproj_err_thr=0", INVALID), ("reproj_err_thr=nan", INVALID),
        ("reproj_err_thr=inf", INVALID), ("parallax_deg_thr=0", INVALID), ("parallax_deg_thr=-1", INVALID), ("parallax_deg_thr=nan", INVALID),
        ("cam1=fx0", INVALID), ("cam1=fy0", INVALID), ("cam1=nanfx", INVALID), ("cam1=inffy", INVALID), ("cam1=nancx", INVALID), ("cam1=equi", INVALID),
        ("P=3:off=0,20,40,60", CAPACITY), ("off=0,101", CAPACITY), ("P=0:off=0", NOTHING), ("P=2:off=0,0,0:models=1,2", ok(0)),
        ("P=3:off=0,20,40,60:cam1=fx0", CAPACITY), ("off=0,101:models=3", CAPACITY), ("P=0:off=0:reproj_err_thr=0", INVALID), ("h=0:P=0:off=0", INVALID)]),
    "triangulate": ("", HEAD_ROWS + [("null=%s" % k, INVALID) for k in (
        "cams_1", "cams_2", "poses_cw_1", "poses_cw_2", "out_pos_w", "out_status", "out_method", "out_num_accepted", "bearings_1", "bearings_2", "keypts_1",
        "keypts_2", "x_right_1", "x_right_2", "depths_1", "depths_2", "sigma_sq_1", "sigma_sq_2", "scale_factors_1", "scale_factors_2")] + [
        ("cos_rays_parallax_thr=nan", INVALID), ("cos_rays_parallax_thr=inf", INVALID), ("ratio_factor=nan", INVALID), ("ratio_factor=inf", INVALID)] + [
        ("%s=%s" % (side, bad), INVALID) for side in ("cam1", "cam2") for bad in ("model2", "nanfx", "inffy", "nancx", "fx0", "fy0", "norows", "nocols")] + [
        ("P=3:off=0,20,40,60", CAPACITY), ("off=0,71", CAPACITY), ("P=0:off=0", NOTHING), ("P=2:off=0,0,0", ok(0)),
        ("P=2:off=0,0,0:null=bearings_1+out_pos_w+out_status", ok(0)), ("P=2:off=0,0,0:null=out_num_accepted", INVALID),
        ("P=3:off=0,20,40,60:cam2=fy0", CAPACITY), ("P=0:off=0:ratio_factor=nan", INVALID), ("h=0:P=0:off=0", INVALID)]),
    # a handle of 8 landmarks, 140 observations, 6 keyframes; one landmark of nine observations over four keyframes
    "landmarks": ("maxp=8:maxt=140:maxk=6:off=0,9:K=4", [
        ("", ok(9)), ("h=0", INVALID), ("off=-", INVALID)] + [("null=%s" % k, INVALID) for k in (
            "pos_w", "ref_keyfrm", "ref_level", "obs_keyfrm", "obs_desc", "cam_centers", "scale_factors", "out_mean_normal", "out_min_max_dist", "out_best_obs",
            "out_desc", "out_status")] + [
        ("what=0", INVALID), ("what=4", INVALID), ("P=-1", INVALID), ("off=1,9", INVALID), ("P=2:off=0,9,5", INVALID), ("levels=0", INVALID), ("levels=17", INVALID),
        ("levels=16", ok(9)), ("okf=0,1,2,3,0,1,2,3,4", INVALID), ("okf=0,1,2,3,0,1,2,3,-1", INVALID), ("refk=6", INVALID), ("refk=4", INVALID), ("refk=-1", INVALID),
        ("refk=3", ok(9)), ("K=3:okf=0,1,2,3,0,1,2,3,0", INVALID), ("K=3", ok(9)), ("refl=8", INVALID), ("refl=-1", INVALID), ("refl=3:levels=3", INVALID), ("refl=7", ok(9)),
        ("P=9:off=0,1,2,3,4,5,6,7,8,9", CAPACITY), ("off=0,141", CAPACITY), ("K=7", CAPACITY), ("K=6", ok(9)), ("P=0:off=0", NOTHING), ("P=2:off=0,0,0", ok(0)),
        ("what=2:K=0:levels=0:null=pos_w+ref_keyfrm+ref_level+obs_keyfrm+cam_centers+scale_factors+out_mean_normal+out_min_max_dist", ok(9)),
        ("what=1:null=obs_desc+out_best_obs+out_desc", ok(9)), ("what=1:null=obs_keyfrm", INVALID),
        ("K=7:refl=-1", CAPACITY), ("K=7:okf=0,1,2,3,0,1,2,3,9", CAPACITY), ("K=-1", INVALID), ("K=-1:P=9:off=0,1,2,3,4,5,6,7,8,9", INVALID),
        ("levels=0:off=0,141", INVALID), ("what=2:K=7", ok(9)), ("what=2:K=-1", ok(9)), ("P=0:off=0:what=0", INVALID), ("P=0:off=0:levels=0", NOTHING),
        # the _f form: the descriptors come from the resident keyframes
        ("res=1", ok(9)), ("res=1:null=keyfrms", INVALID), ("res=1:null=obs_keypoint", INVALID), ("res=1:null=obs_keyfrm", INVALID),
        ("res=1:kfdev=0,-1,0,0", INVALID), ("res=1:kfdev=0,1,0,0", INVALID), ("res=1:dev=1", INVALID), ("res=1:dev=1:kfdev=1,1,1,1", ok(9)),
        ("res=1:kfdev=0,0,0,0,-1", ok(9)), ("res=1:okp=0,1,2,3,4,5,6,7,100", INVALID), ("res=1:okp=0,1,2,3,4,5,6,7,-1", INVALID),
        ("res=1:okp=0,1,2,3,4,5,6,7,99", ok(9)), ("res=1:kfn=100,100,100,5:okp=0,1,2,5,0,0,0,0,0", INVALID), ("res=1:kfn=100,100,100,5:okp=0,1,2,4,0,0,0,4,0", ok(9)),
        ("res=1:what=1:null=keyfrms+obs_keypoint", ok(9)), ("res=1:what=2:null=obs_keyfrm", INVALID), ("res=1:what=2:K=7", CAPACITY),
        ("res=1:what=2:K=-1", INVALID), ("res=1:K=7:kfdev=0,-1", CAPACITY)]),
}


def check_row(fam, keys):
    base = CONTRACTS[fam][0]
    return "check:" + ":".join(x for x in (fam, base, keys) if x)


# ---- staging: two problems of 2 and 3 matches; input array number `id` holds id * 16 + i at element i
STAGE = "P=2:off=0,2,5:maxp=2:maxt=5"


def pat(n, ident):
    return [ident * 16 + i for i in range(n)]


def f64(v):
    return struct.pack("<%dd" % len(v), *[float(x) for x in v])


def f32(v):
    return struct.pack("<%df" % len(v), *[float(x) for x in v])


def i32(v):
    return struct.pack("<%di" % len(v), *v)


def u8(v):
    return bytes(x & 255 for x in v)


def block(n, *parts):
    b = bytearray(b"\xee" * n)   # 0xee: what the program fills the heap buffer with before staging
    for off, data in parts:
        assert off + len(data) <= n
        b[off:off + len(data)] = data
    return bytes(b).hex() if n else "-"


def at(fam, P, T, name):
    return {s[0]: s[1] for s in LAYOUTS[fam](P, T)[0]}[name]


def cam_ok(p):      # a, b, c, d, model, pad of the program's camera "ok" of problem p
    return struct.pack("<4d2i", 458 + p, 457 + p, 367 + p, 248 + p, 0, 0)


def cam_equi(p):    # "equi": (double)cols, (double)rows, 0, 0
    return struct.pack("<4d2i", 1920 + p, 960 + p, 0, 0, 1, 0)


def planes(v, width):   # [T][width] -> [width][T]
    return [v[width * i + x] for x in range(width) for i in range(len(v) // width)]


def stage_sim3():
    L = lambda n: at("sim3", 2, 5, n)
    return "476 " + block(476, (L("keys"), bytes(16)), (L("cams"), cam_ok(0) + cam_equi(0) + cam_ok(1) + cam_equi(1)), (L("p1"), f64(pat(15, 1))),
                          (L("p2"), f64(pat(15, 2))), (L("thr1"), f32(pat(5, 3))), (L("thr2"), f32(pat(5, 4))), (L("offsets"), i32([0, 2, 5])))


def stage_pnp():
    L = lambda n: at("pnp", 2, 5, n)
    return "308 " + block(308, (0, bytes(16)), (L("bearings"), f64(pat(15, 1))), (L("pos_w"), f64(pat(15, 2))), (L("max_cos"), f64(pat(5, 3))),
                          (L("offsets"), i32([0, 2, 5])))


def stage_sim3opt():
    L = lambda n: at("sim3opt", 2, 5, n)
    init = b"".join(f64(pat(18, 7)[9 * p:9 * p + 9] + pat(6, 8)[3 * p:3 * p + 3] + [pat(2, 9)[p]]) for p in range(2))
    return "833 " + block(833, (0, cam_ok(0) + cam_equi(0) + cam_ok(1) + cam_equi(1)), (L("init"), init), (L("p1"), f64(pat(15, 1))), (L("p2"), f64(pat(15, 2))),
                          (L("obs1"), f64(pat(10, 3))), (L("obs2"), f64(pat(10, 4))), (L("w1"), f32(pat(5, 5))), (L("w2"), f32(pat(5, 6))),
                          (L("offsets"), i32([0, 2, 5])), (L("work"), bytes(5)))


def stage_twoview():
    return "172 " + block(172, (0, f64(pat(10, 1))), (80, f64(pat(10, 2))), (160, i32([0, 2, 5])))


def stage_essential():
    return "252 " + block(252, (0, f64(pat(15, 1))), (120, f64(pat(15, 2))), (240, i32([0, 2, 5])))


def stage_reconstruct():
    L = lambda n: at("reconstruct", 2, 5, n)
    problems = b"".join(f64(pat(18, 1)[9 * p:9 * p + 9] + [458 + p, 457 + p, 367 + p, 248 + p]) + i32([1 + p, 0]) for p in range(2))   # models 1, 2
    return "641 " + block(641, (0, problems), (L("kp1"), f64(pat(10, 3))), (L("kp2"), f64(pat(10, 4))), (L("b1"), f64(pat(15, 5))), (L("b2"), f64(pat(15, 6))),
                          (L("offsets"), i32([0, 2, 5])), (L("inlier"), u8(pat(5, 2))))


def stage_triangulate():
    L = lambda n: at("triangulate", 2, 5, n)
    problems = b""
    for p in range(2):
        poses = [pat(24, 13)[12 * p:12 * p + 12], pat(24, 14)[12 * p:12 * p + 12]]
        centres = [-float((q[c] * q[9] + q[3 + c] * q[10]) + q[6 + c] * q[11]) for q in poses for c in range(3)]   # -R^T t, dot3's order
        problems += struct.pack("<6d2i", 458 + p, 457 + p, 367 + p, 248 + p, 40 + p, 0.5 + p, 0, 0)
        problems += struct.pack("<6d2i", 1920 + p, 960 + p, 0, 0, 40 + p, 0.5 + p, 1, 0)
        problems += f64(poses[0] + poses[1]) + f64(centres)
    fl = L("f32")
    floats = [(fl + 24 * k, f32(v)) for k, v in enumerate(
        [planes(pat(10, 3), 2)[:5], planes(pat(10, 3), 2)[5:], planes(pat(10, 4), 2)[:5], planes(pat(10, 4), 2)[5:]] + [pat(5, ident) for ident in range(5, 13)])]
    staged = block(1402, (0, problems), (L("b1"), f64(planes(pat(15, 1), 3))), (L("b2"), f64(planes(pat(15, 2), 3))), *floats,
                   (L("pidx"), i32([0, 0, 1, 1, 1])), (L("offsets"), i32([0, 2, 5])))
    # collect: pos [3][T] = 1000 + i, status i % 3, method 80 + i
    pos = f64([1000 + x * 5 + i for i in range(5) for x in range(3)]).hex()
    return " ".join(["1402", staged, pos, u8([0, 1, 2, 0, 1]).hex(), u8([80 + i for i in range(5)]).hex(), i32([1, 1]).hex()])


def landmark_answer(P, T, with_desc, parts, n8, n64, table_parts, normal, rng, best, desc, status):
    sections, (total, nbytes) = lay_landmarks(P, T, with_desc)
    L = {s[0]: s[1] for s in sections}
    return " ".join(["%d %d" % (nbytes, total), block(total, *[(L[name], data) for name, data in parts]), "%d %d" % (n8, n64), block(192, *table_parts),
                     f64(normal).hex(), f32(rng).hex(), i32(best).hex(), u8(desc).hex(), u8(status).hex()])


COLLECTED_2 = dict(normal=[1000 + x * 2 + p for p in range(2) for x in range(3)], rng=[2000, 2002, 2001, 2003], best=[1, 1],
                   desc=[120 + i for i in range(64)], status=[0, 0])


def stage_landmarks():
    parts = [("pos", f64(planes(pat(6, 1), 3))), ("sf_ref", f32([64, 65])), ("ref_slot", i32([0, 0])), ("offsets", i32([0, 2, 5])),
             ("obs_slot", i32([0, 1, 2, 0, 1])), ("used", i32([0, 1, 2, 3, 4])), ("n_used", i32([2, 3])), ("list8", i32([0, 1])), ("desc", u8(pat(160, 2)))]
    return landmark_answer(2, 5, True, parts, 2, 0, [(0, f64(pat(9, 3)))], **COLLECTED_2)


def stage_landmarks_resident():
    parts = [("pos", f64(planes(pat(6, 1), 3))), ("sf_ref", f32([64, 65])), ("ref_slot", i32([0, 0])), ("offsets", i32([0, 2, 5])),
             ("obs_slot", i32([0, 1, 2, 0, 1])), ("used", i32([0, 1, 2, 3, 4])), ("n_used", i32([2, 3])), ("list8", i32([0, 1])), ("obs_kp", i32([0, 1, 2, 3, 4]))]
    table = [(0, f64(pat(9, 3))), (72, bytes([1] * 8 + [2] * 8 + [3] * 8))]   # the program prints pointer k as eight bytes of k + 1
    return landmark_answer(2, 5, False, parts, 2, 0, table, **COLLECTED_2)


MIXED = "P=3:off=0,4,13,13:maxp=3:maxt=13:use=1,1,0,1,1,1,1,1,1,1,1,1,1"


def stage_landmarks_mixed():
    """One landmark of four observations with the third switched off, one of nine, one empty."""
    parts = [("pos", f64(planes(pat(9, 1), 3))), ("sf_ref", f32([64, 65, 0])), ("ref_slot", i32([0, 0, 0])), ("offsets", i32([0, 4, 13, 13])),
             ("obs_slot", i32([t % 3 for t in range(13)])), ("used", i32([0, 1, 3])), ("n_used", i32([3, 9, 0])), ("list8", i32([0])), ("list64", i32([1])),
             ("desc", u8(pat(416, 2)))]
    used_at = at("landmarks:desc=1", 3, 13, "used")
    sections, (total, nbytes) = lay_landmarks(3, 13, True)
    L = {s[0]: s[1] for s in sections}
    blk = block(total, *[(L[n], d) for n, d in parts], (used_at + 16, i32(list(range(4, 13)))))   # the second landmark's list starts at its offset, 4
    return " ".join(["%d %d" % (nbytes, total), blk, "1 1", block(192, (0, f64(pat(9, 3)))),
                     f64([1000, 1003, 1006, 1001, 1004, 1007, -7, -7, -7]).hex(), f32([2000, 2003, 2001, 2004, -7, -7]).hex(), i32([1, 1, -7]).hex(),
                     u8([120 + i for i in range(64)] + [9] * 32).hex(), u8([0, 0, 1]).hex()])


STAGED = {"stage:sim3:" + STAGE: stage_sim3, "stage:pnp:" + STAGE: stage_pnp, "stage:sim3opt:" + STAGE: stage_sim3opt, "stage:twoview:" + STAGE: stage_twoview,
          "stage:essential:" + STAGE: stage_essential, "stage:reconstruct:" + STAGE: stage_reconstruct, "stage:triangulate:" + STAGE: stage_triangulate,
          "stage:landmarks:" + STAGE: stage_landmarks, "stage:landmarks:res=1:" + STAGE: stage_landmarks_resident, "stage:landmarks:" + MIXED: stage_landmarks_mixed}


def all_rows():
    rows = [layout_row(k, P, T) for k in LAYOUTS for P, T in SIZES]
    rows += [check_row(fam, keys) for fam, (_, table) in CONTRACTS.items() for keys, _ in table]
    return rows + list(STAGED)


def run_rows(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    return dict(zip(rows, lines))


@pytest.fixture(scope="module")
def answers():
    subprocess.check_call(["make", "-s", "-C", CPP, "solve_plan_host"])
    return run_rows(EXE, all_rows())


@pytest.mark.parametrize("key", list(LAYOUTS))
def test_layouts(answers, key):
    """Every offset as the unit's layout_of computed it; element alignment; sections in order, disjoint and inside what the call uploads or reads back;
    a larger call never needs a smaller block."""
    sizes = {}
    for P, T in SIZES:
        sections, tail = LAYOUTS[key](P, T)
        assert [int(v) for v in answers[layout_row(key, P, T)].split()] == [s[1] for s in sections] + tail, (P, T)
        end = tail[0]   # bytes; total for the landmark block
        for (name, off, size, align), nxt in zip(sections, sections[1:] + [("end", end, 0, 1)]):
            assert off % align == 0 and off + size <= nxt[1], (P, T, name)
        if key.startswith("landmarks"):
            assert tail[1] <= tail[0] and tail[1] == dict((s[0], s[1]) for s in sections)["normal" if key.endswith("1") else "desc"]
        sizes[(P, T)] = end
    for (P, T), n in sizes.items():
        for (P2, T2), n2 in sizes.items():
            assert not (P2 >= P and T2 >= T) or n <= n2, (P, T, P2, T2)


@pytest.mark.parametrize("fam", list(CONTRACTS))
def test_error_contracts(answers, fam):
    for keys, want in CONTRACTS[fam][1]:
        want = want if isinstance(want, tuple) else (want, 0, 0)
        assert tuple(int(v) for v in answers[check_row(fam, keys)].split()) == want, keys


@pytest.mark.parametrize("row", list(STAGED), ids=["sim3", "pnp", "sim3opt", "twoview", "essential", "reconstruct", "triangulate", "landmarks", "landmarks_resident", "landmarks_mixed"])
def test_staging(answers, row):
    """Every byte of the block: the sections hold their inputs in the layout's order (plane-transposed where the kernels read planes), nothing is
    written between or behind them; and what collect hands the caller from output sections filled with a pattern."""
    assert answers[row] == STAGED[row]()


def test_the_program_refuses_a_malformed_row(answers):
    for row in ("layout:sim3:P=0:T=1", "layout:nothing:P=1:T=1", "check:sim3:P=x", "check:sim3:cam1=fisheye", "check:sim3:P=2", "stage:sim3:h=0",
                "plan:sim3", "check"):
        assert subprocess.run([EXE], input=row + "\n", capture_output=True, text=True, timeout=60).returncode == 2, row


def test_host_program_runs_clean_under_the_sanitizers(answers):
    """A stand-alone program with its own main on this CPU, AddressSanitizer and UndefinedBehaviorSanitizer linked in: the same rows, the same
    answers. Each staged block is a heap buffer of exactly the layout's bytes, so a copy past a section's end at the block's end lands in a red
    zone. The test puts nothing into the child's environment and takes nothing out of it."""
    subprocess.check_call(["make", "-s", "-C", CPP, "solve_plan_host_san"])
    assert run_rows(os.path.join(CPP, "solve_plan_host_san"), all_rows()) == answers
