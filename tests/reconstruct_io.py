"""Files and arrays of the pose-recovery tests: the case file tests/reconstruct_host.cc and cpp/test_reconstruct_shim.cc read, and what they
write back. A problem is a dict as tests/reconstruct_ref.py takes it."""
import struct

import numpy as np


def host_input(problems, reproj_err_thr=4.0, parallax_deg_thr=1.0, min_num_triangulated=50):
    out = [struct.pack("<ffii", reproj_err_thr, parallax_deg_thr, min_num_triangulated, len(problems))]
    for q in problems:
        out.append(struct.pack("<i9d4di", q["model"], *q["mat"], *q["cam"], len(q["inlier"])))
        for i, flag in enumerate(q["inlier"]):
            out.append(struct.pack("<B10d", flag, *q["kp1"][i], *q["kp2"][i], *q["b1"][i], *q["b2"][i]))
    return b"".join(out)


def host_output(text, sizes):
    """The program's lines as the dicts reconstruct_ref.as_bits returns."""
    lines = text.split("\n")
    out, k = [], 0
    for n in sizes:
        head, counts, angles = lines[k].split(), lines[k + 1].split(), lines[k + 2].split()
        assert head[0] == "P" and counts[0] == "C" and angles[0] == "A", lines[k:k + 3]
        r = dict(success=int(head[1]), best=int(head[2]), R=[int(v, 16) for v in head[3:12]], t=[int(v, 16) for v in head[12:15]],
                 counts=[int(v) for v in counts[1:]], parallax=[_float_bits_as_double_bits(int(v, 16)) for v in angles[1:]], pts=[], flags=[])
        for line in lines[k + 3:k + 3 + n]:
            w = line.split()
            assert w[0] == "M", line
            r["flags"].append(int(w[1]))
            r["pts"].append([int(v, 16) for v in w[2:5]])
        out.append(r)
        k += 3 + n
    return out


def _float_bits_as_double_bits(u):
    return struct.unpack("<Q", struct.pack("<d", struct.unpack("<f", struct.pack("<I", u))[0]))[0]


def write_shim_scene(path, two_view_problems, cam, num_ransac_iters, seed, reproj_err_thr=4.0, parallax_deg_thr=1.0, min_num_triangulated=50):
    """What cpp/test_reconstruct_shim.cc reads: the matched keypoints of every (reference, current) pair, as floats."""
    out = [struct.pack("<ffiiQ4di", reproj_err_thr, parallax_deg_thr, min_num_triangulated, num_ransac_iters, seed, *cam, len(two_view_problems))]
    for q in two_view_problems:
        n = len(q["x1"])
        out.append(struct.pack("<i", n))
        out.append(np.array(q["x1"], np.float32).reshape(n, 2).tobytes())
        out.append(np.array(q["x2"], np.float32).reshape(n, 2).tobytes())
    with open(path, "wb") as f:
        f.write(b"".join(out))


def read_shim_results(path, sizes):
    """Per problem: dict initialised, R, t (bit patterns), pts (bit patterns) and flags by the reference frame's keypoint."""
    data = open(path, "rb").read()
    out, k = [], 0
    for n in sizes:
        ok, = struct.unpack_from("<i", data, k)
        pose = struct.unpack_from("<12Q", data, k + 4)
        m, = struct.unpack_from("<i", data, k + 100)
        assert m == n + 5, (m, n)
        k += 104
        pts, flags = [], []
        for _ in range(m):
            pts.append(list(struct.unpack_from("<3Q", data, k)))
            flags.append(data[k + 24])
            k += 25
        out.append(dict(initialised=ok, R=list(pose[:9]), t=list(pose[9:]), pts=pts, flags=flags))
    assert k == len(data)
    return out


def device_problem(q):
    """A reference problem as openvslam_amd.solve.reconstruct_two_view_batch takes it."""
    from openvslam_amd import solve
    n = len(q["inlier"])
    fx, fy, cx, cy = q["cam"]
    return solve.reconstruct_problem(q["model"], np.array(q["mat"], np.float64).reshape(3, 3), solve.camera(0, fx, fy, cx, cy), np.array(q["inlier"], np.uint8),
                                     np.array(q["kp1"], np.float64).reshape(n, 2), np.array(q["kp2"], np.float64).reshape(n, 2),
                                     np.array(q["b1"], np.float64).reshape(n, 3), np.array(q["b2"], np.float64).reshape(n, 3))


def of_device(r):
    """A result of reconstruct_two_view_batch as reconstruct_ref.as_bits returns the reference's."""
    bits = lambda a: [int(v) for v in np.ascontiguousarray(a, np.float64).ravel().view(np.uint64)]
    pts = np.ascontiguousarray(r["triangulated_pts"], np.float64).reshape(-1, 3)
    return dict(success=int(r["success"]), best=int(r["best"]), R=bits(r["rot_ref_to_cur"]), t=bits(r["trans_ref_to_cur"]), counts=[int(v) for v in r["counts"]],
                parallax=bits(np.asarray(r["parallax_deg"], np.float32).astype(np.float64)), pts=[bits(p) for p in pts],
                flags=[int(v) for v in r["is_triangulated"]])
