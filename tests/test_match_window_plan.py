"""The window matchers' host plan (openvslam_amd/csrc/match_window_plan.inc) without a device: tests/match_window_plan_host.cc, built by the plain
host compiler from the plan alone, prints what the plan decides for the rows below. The expected values are written out by hand from the conditions
match_window.hip held before the plan was moved out of it (launch_resolve, launch_grid_assign, dead_from_ratio, ovs_frame_dev_create, the three sums
of ovs_wmatcher_create and the stg.put / stg.reserve sequence of every *_impl), not generated from the plan; the pose helpers are held, bit for bit,
to a numpy restatement that spells out the same operation order. The GPU tests see results only; which launch form ran, and that the staging arena
has room for every entry point at full capacity, is visible here."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
EXE = os.path.join(CPP, "match_window_plan_host")
KIB = 1024


def fhex(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


def dhex(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def dbits(a):
    return [dhex(float(v)) for v in np.asarray(a, np.float64).ravel()]


# ---- resolver: (n_q, n_t, wide_from) -> (ok, fixed bytes, offsets_in_lds, lds bytes, key_pool, width) -----------------------------------------
# fixed = 4096 * 4 + 32 * 4 + 4 * even(n_t) + 4 * even(n_q); offsets (4 * ((n_q + 4) & ~3) bytes) join it while the sum stays <= 120 KiB; the
# allocation is min(150 KiB, max(96 KiB, fixed + 24 KiB)); key_pool = the words left; width 0 / 1 / 2 = 1 / 4 / 8 waves
RESOLVE = [
    ((256, 2000, 1024), (1, 25536, 1, 96 * KIB, 17932, 0)),         # the 96 KiB floor binds
    ((257, 2000, 1024), (1, 25544, 1, 96 * KIB, 17930, 1)),
    ((1024, 2000, 1024), (1, 28608, 1, 96 * KIB, 16396, 1)),
    ((1025, 2000, 1024), (1, 28616, 1, 96 * KIB, 16394, 2)),
    ((1025, 2000, 2048), (1, 28616, 1, 96 * KIB, 16394, 1)),        # wide_from overridden
    ((2049, 2000, 2048), (1, 32712, 1, 96 * KIB, 14346, 2)),
    ((12295, 2000, 1024), (1, 73696, 1, 144 * KIB, 6144, 2)),       # the last with the list bounds in LDS: 73696 + 49184 = 120 KiB; fixed + 24 KiB binds
    ((12296, 2000, 1024), (1, 73696, 0, 96 * KIB, 6152, 2)),        # the first without: 73696 + 49200 > 120 KiB; the floor binds again
    ((17136, 17136, 1024), (1, 150 * KIB, 0, 150 * KIB, 0, 2)),     # the last size accepted: fixed = 150 KiB, no room for keys
    ((17137, 17136, 1024), (0, 150 * KIB + 8, 0, 0, 0, 0)),         # the first refused
    ((1, 34000, 1024), (1, 152520, 0, 150 * KIB, 270, 0)),          # the edge ovs_wmatcher_create still accepts, either way round
    ((34000, 1, 1024), (1, 152520, 0, 150 * KIB, 270, 2)),
]

# ---- grid launch: (n, cells) -> (items_in_lds, lds bytes, attribute raised) -------------------------------------------------------------------
GRID = [
    ((8192, 64 * 48), (1, 57348, 0)),
    ((8193, 64 * 48), (0, 24580, 0)),
    ((4095, 16384), (1, 144 * KIB, 1)),      # (2 * 16384 + 1 + 4095) * 4 = 144 KiB: the last that fits
    ((4096, 16384), (0, 131076, 1)),
    ((8191, 4096), (1, 64 * KIB, 0)),        # the 64 KiB a kernel gets without the attribute
    ((8192, 4096), (1, 64 * KIB + 4, 1)),
    ((0, 1), (1, 12, 0)),
]
# (cols, rows, min_x, min_y, max_x, max_y) -> grid_params_ok
GRID_OK = [
    ((128, 128, 0.0, 0.0, 752.0, 480.0), 1),      # 16384 cells
    ((145, 113, 0.0, 0.0, 752.0, 480.0), 0),      # 16385
    ((64, 48, 10.0, 0.0, 10.0, 480.0), 0),        # max_x == min_x
    ((64, 48, 0.0, 5.0, 752.0, 5.0), 0),
    ((0, 48, 0.0, 0.0, 752.0, 480.0), 0),
    ((64, 48, -3.5, -2.25, 755.5, 482.25), 1),
]

# ---- dead-candidate thresholds: the smallest d > thr with fl(d * ratio) >= thr, 257 if there is none --------------------------------------------
DEAD = [
    ((50, 0.6), 84), ((50, 0.75), 67), ((50, 0.9), 56), ((50, 1.0), 51),
    ((100, 0.6), 167), ((100, 0.75), 134), ((100, 0.9), 112), ((100, 1.0), 101),
    ((100, 0.3), 257),
    ((50, 0.0), 257), ((50, -0.8), 257), ((100, float("nan")), 257),
]

# ---- frame arena: (n, stereo) -> cap, six offsets, arena bytes, upload bytes, pinned staging bytes ---------------------------------------------
# keypoints 28 B | descriptors 32 B | stereo_x_right 4 B | cell_of 4 B | items 4 B per capacity slot, then 16385 cell starts; each on 256 bytes
A4096 = (4096, 0, 114688, 245760, 262144, 278528, 294912, 360704)
A8192 = (8192, 0, 229376, 491520, 524288, 557056, 589824, 655616)
A65536 = (65536, 0, 1835008, 3932160, 4194304, 4456448, 4718592, 4784384)
ARENA = [
    ((0, 0), A4096 + (0, 311296)), ((0, 1), A4096 + (0, 311296)),
    ((1, 0), A4096 + (114720, 311296)), ((1, 1), A4096 + (245764, 311296)),
    ((4096, 0), A4096 + (245760, 311296)), ((4096, 1), A4096 + (262144, 311296)),
    ((4097, 0), A8192 + (360480, 557056)), ((4097, 1), A8192 + (507908, 557056)),
    ((65534, 0), A65536 + (3932096, 3997696)), ((65534, 1), A65536 + (4194296, 4194296)),
]

# ---- staging ----------------------------------------------------------------------------------------------------------------------------------
PAIRS = [(1, 1), (2000, 3000), (8192, 16384), (17000, 17000), (34000, 1), (1, 34000)]
KP = 28   # sizeof(ovs_keypoint)


def capacity(T, Q):
    """ovs_wmatcher_create's three sums, as they stood in match_window.hip."""
    N = min(T, Q)
    window = T * (KP + 32 + 4 + 1) + Q * (KP + 24 + 24 + 8 + 32 + 1 + 8 + 4 + 4 + 8) + 4 * 16 + 15 * 256
    bow = (T + Q) * (KP + 32 + 1 + 4 + 24) + 4 * (4 * (T + Q) + 16) + 16 * 256
    mutual = 2 * N * (KP + 32 + 24 + 8 + 32 + 1 + 4) + 14 * 256
    return max(window, bow, mutual)


def csr_sizes(T, Q):
    """(kf_nodes, nq, frm_nodes, nfi): two feature vectors that fill the documented 4 (T + Q) + 16 ints, the queries within max_queries."""
    sizes = (Q, Q, T, 2 * T + Q + 14)
    assert sizes[0] + sizes[0] + 1 + sizes[1] + sizes[2] + sizes[2] + 1 + sizes[3] == 4 * (T + Q) + 16
    return sizes


def staged(entry, T, Q, resident):
    """The arrays an entry point stages at n == T, m == Q with every optional array present, in order: (bytes, copied). From the *_impl bodies."""
    side = lambda n, xr=False, br=False: [] if resident else [(KP * n, 1), (32 * n, 1)] + [(4 * n, 1)] * xr + [(24 * n, 1)] * br
    scratch = lambda n: [(n, 1), (8 * n, 0), (4 * n, 0), (4 * n, 0), (4 * n, 0), (4 * n, 0)]   # valid flags (copied), then what k_reproject_queries writes
    if entry == "grid":
        return [(KP * T, 1)]
    if entry == "frame_and_landmarks":
        return side(T, xr=True) + [(T, 1), (8 * Q, 1), (4 * Q, 1), (4 * Q, 1), (Q, 1), (32 * Q, 1)]
    if entry == "area":
        return [(8 * Q, 1)] + side(Q) + side(T)
    if entry == "current_and_last":
        return side(T, xr=True) + [(T, 1), (KP * Q, 1), (24 * Q, 1), (32 * Q, 1), (64, 1)] + scratch(Q)
    if entry == "frame_and_keyframe":
        return [(T, 1), (KP * Q, 1), (24 * Q, 1), (8 * Q, 1), (32 * Q, 1), (64, 1)] + scratch(Q) + side(T)
    if entry == "sim3_transform":
        return [(T, 1), (24 * Q, 1), (8 * Q, 1), (24 * Q, 1), (32 * Q, 1), (64, 1)] + scratch(Q) + side(T)
    if entry == "fuse":
        return [(24 * Q, 1), (24 * Q, 1), (8 * Q, 1), (32 * Q, 1), (Q, 1)] + side(T, xr=True)
    if entry == "mutual":
        N = min(T, Q)
        return [(24 * N, 1), (8 * N, 1), (32 * N, 1), (N, 1)] * 2 + [(4 * N, 0)] * 2 + side(N) * 2
    kn, nq, fn, nfi = csr_sizes(T, Q)
    tri = entry == "tri"
    if tri and resident:   # the handles carry stereo_x_right and bearings
        sides = []
    else:
        sides = side(Q, xr=tri, br=tri) + side(T, xr=tri, br=tri)
    return sides + [(Q, 1), (4 * kn, 1), (4 * (kn + 1), 1), (4 * nq, 1), (T, 1), (4 * fn, 1), (4 * (fn + 1), 1), (4 * nfi, 1)]


ENTRIES = ["grid", "frame_and_landmarks", "area", "current_and_last", "frame_and_keyframe", "sim3_transform", "fuse", "mutual", "bow", "tri"]
# arrays of the three calls the capacity sums are written for, host form: against 15, 16 and 14 x 256 bytes of alignment slack
N_ARRAYS = {"frame_and_keyframe": 14, "current_and_last": 14, "sim3_transform": 14, "tri": 16, "mutual": 14}


def stage_row(entry, T, Q, resident):
    row = "stage:%s:%d:%d:%d" % (entry, T, Q, resident)
    return row + ":%d:%d:%d:%d" % csr_sizes(T, Q) if entry in ("bow", "tri") else row


STAGE = [(e, T, Q, r) for e in ENTRIES for (T, Q) in PAIRS for r in (0, 1) if not (e == "grid" and r)]

# ---- pose helpers -----------------------------------------------------------------------------------------------------------------------------


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def _pose(angles, t, scale=1.0):
    return np.concatenate([(scale * _rot(*angles)).ravel(), np.asarray(t, np.float64)])   # 9 + 3 doubles, row-major rotation first


POSES = [
    _pose((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    _pose((0.1, -0.2, 0.3), (0.5, -1.25, 2.0)),
    _pose((-1.3, 0.7, 2.9), (-13.7, 0.001, 4.4)),
    _pose((0.02, 0.01, -0.03), (0.05, 0.02, -0.9)),          # a translation along -z beyond the baseline below
    _pose((0.4, 0.5, -0.6), (1.0, 2.0, 3.0), scale=2.5),     # a scale other than 1 (a Sim3)
    _pose((-0.7, 0.2, 0.1), (0.3, -0.1, 0.7), scale=0.37),
]
BASELINE = 0.12


def np_camera_centre(P):
    P = np.asarray(P, np.float64)
    return [-((P[i] * P[9] + P[3 + i] * P[10]) + P[6 + i] * P[11]) for i in range(3)]


def np_decompose_sim3(S):
    S = np.asarray(S, np.float64)
    sc = np.sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2])
    P = S / sc
    return list(P) + np_camera_centre(P)


def np_motion(setup, cur, last):
    twc = np_camera_centre(cur)
    last = np.asarray(last, np.float64)
    z = ((last[6] * twc[0] + last[7] * twc[1]) + last[8] * twc[2]) + last[11]
    return (0, 0) if setup == 0 else (int(z > BASELINE), int(-z > BASELINE))


def np_two_way(s, R, t):
    s, R, t = np.float64(s), np.asarray(R, np.float64), np.asarray(t, np.float64)
    S12 = [s * R[i] for i in range(9)] + list(t)
    inv = np.float64(1.0) / s
    S21 = [inv * R[3 * c + r] for r in range(3) for c in range(3)]
    S21 += [-((S21[3 * r] * t[0] + S21[3 * r + 1] * t[1]) + S21[3 * r + 2] * t[2]) for r in range(3)]
    return S12 + S21


def np_gridp(cols, rows, min_x, min_y, max_x, max_y):
    f = np.float32
    inv_w = f(np.float64(cols) / np.float64(f(max_x) - f(min_x)))   # a float difference, a double division, narrowed to float
    inv_h = f(np.float64(rows) / np.float64(f(max_y) - f(min_y)))
    return [fhex(f(min_x)), fhex(f(min_y)), fhex(inv_w), fhex(inv_h), str(cols), str(rows)]


GRIDP = [(64, 48, 0.0, 0.0, 752.0, 480.0), (64, 48, -3.5, -2.25, 755.5, 482.25), (64, 48, 0.0, 0.0, 3840.0, 1920.0), (96, 54, 12.7, 3.1, 1907.3, 1076.9),
         (7, 3, 0.0, 0.0, 0.3, 0.7)]
TWO_WAY = [(1.0, POSES[0]), (1.0, POSES[1]), (2.5, POSES[2]), (0.37, POSES[3]), (1.0 / 3.0, POSES[1])]   # (s_12, [R_12 | t_12])
MOTION = [(setup, c, l) for setup in (0, 1, 2) for (c, l) in ((0, 1), (1, 0), (3, 0), (0, 3), (2, 1), (0, 0))]


def helper_rows():
    """row -> the fields numpy expects"""
    rows = {}
    for g in GRIDP:
        rows["gridp:%d:%d:%s" % (g[0], g[1], ":".join(fhex(v) for v in g[2:]))] = np_gridp(*g)
    for P in POSES:
        rows["centre:" + ":".join(dbits(P))] = dbits(np_camera_centre(P))
        rows["sim3:" + ":".join(dbits(P))] = dbits(np_decompose_sim3(P))
    for s, P in TWO_WAY:
        R = P[:9] / np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2])
        rows["twoway:%s:%s" % (dhex(s), ":".join(dbits(R) + dbits(P[9:])))] = dbits(np_two_way(s, R, P[9:]))
    for setup, c, l in MOTION:
        rows["motion:%d:%s:%s" % (setup, dhex(BASELINE), ":".join(dbits(POSES[c]) + dbits(POSES[l])))] = [str(v) for v in np_motion(setup, POSES[c], POSES[l])]
    return rows


HELPERS = helper_rows()


@pytest.fixture(scope="module")
def answers():
    subprocess.check_call(["make", "-s", "-C", CPP, "match_window_plan_host"])
    rows = (["resolve:%d:%d:%d" % k for k, _ in RESOLVE] + ["grid:%d:%d" % k for k, _ in GRID]
            + ["gridok:%d:%d:%s" % (k[0], k[1], ":".join(fhex(v) for v in k[2:])) for k, _ in GRID_OK]
            + ["dead:%d:%s" % (t, fhex(r)) for (t, r), _ in DEAD] + ["deadthr:50", "deadthr:100", "pad:8:1", "pad:16:1", "pad:3:0"]
            + ["arena:%d:%d" % k for k, _ in ARENA] + ["capacity:%d:%d" % p for p in PAIRS] + list(HELPERS) + [stage_row(*s) for s in STAGE])
    r = subprocess.run([EXE] + rows, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    return {row: line.split() for row, line in zip(rows, lines)}


def ints(fields):
    return tuple(int(v) for v in fields)


@pytest.mark.parametrize("key,want", RESOLVE, ids=["q%d_t%d_w%d" % k for k, _ in RESOLVE])
def test_resolver_plan(answers, key, want):
    assert ints(answers["resolve:%d:%d:%d" % key]) == want


@pytest.mark.parametrize("key,want", GRID, ids=["n%d_c%d" % k for k, _ in GRID])
def test_grid_launch_plan(answers, key, want):
    assert ints(answers["grid:%d:%d" % key]) == want


def test_grid_params_ok(answers):
    for k, want in GRID_OK:
        assert ints(answers["gridok:%d:%d:%s" % (k[0], k[1], ":".join(fhex(v) for v in k[2:]))]) == (want,), k


def test_dead_thresholds(answers):
    for (thr, ratio), want in DEAD:
        assert ints(answers["dead:%d:%s" % (thr, fhex(ratio))]) == (want,), (thr, ratio)
    assert ints(answers["deadthr:50"]) == (51,) and ints(answers["deadthr:100"]) == (101,)


def test_pad_levels(answers):
    assert [float(v) for v in answers["pad:8:1"]] == [1, 2, 3, 4, 5, 6, 7, 8] + [0.5] * 8
    assert [float(v) for v in answers["pad:16:1"]] == list(range(1, 17))
    assert [float(v) for v in answers["pad:3:0"]] == [0.5] * 16


@pytest.mark.parametrize("key,want", ARENA, ids=["n%d_stereo%d" % k for k, _ in ARENA])
def test_frame_arena(answers, key, want):
    got = ints(answers["arena:%d:%d" % key])
    assert got == want
    cap, offs, arena_bytes, upload = got[0], got[1:7], got[7], got[8]
    assert cap % 4096 == 0 and cap >= max(key[0], 1) and cap - key[0] < 4096 + (key[0] == 0)
    assert all(o % 256 == 0 for o in offs) and list(offs) == sorted(set(offs)) and arena_bytes % 256 == 0
    sizes = (KP * cap, 32 * cap, 4 * cap, 4 * cap, 4 * cap, 4 * 16385)
    assert all(o + s <= nxt for o, s, nxt in zip(offs, sizes, offs[1:] + (arena_bytes,)))
    assert upload <= offs[3]   # the one upload ends before the grid's arrays


@pytest.mark.parametrize("row", list(HELPERS), ids=["%s_%d" % (r.split(":")[0], i) for i, r in enumerate(HELPERS)])
def test_pose_helpers_bit_for_bit(answers, row):
    assert answers[row] == HELPERS[row]


@pytest.mark.parametrize("T,Q", PAIRS)
def test_stage_capacity_is_the_three_sums(answers, T, Q):
    assert ints(answers["capacity:%d:%d" % (T, Q)]) == (capacity(T, Q),)


@pytest.mark.parametrize("entry,T,Q,resident", STAGE, ids=["%s_%d_%d_%s" % (e, T, Q, "resident" if r else "host") for e, T, Q, r in STAGE])
def test_staging_fits_the_arena(answers, entry, T, Q, resident):
    f = answers[stage_row(entry, T, Q, resident)]
    need, cap, overflow = int(f[0]), int(f[1]), int(f[2])
    placed = [p.split(",") for p in f[3:]]
    want = staged(entry, T, Q, resident)
    if not resident and entry in N_ARRAYS:
        assert len(want) == N_ARRAYS[entry]
    # every array where the *_impl put it: on the next 256-byte boundary behind the one before, its bytes there (reserved arrays are not copied)
    off, used, expect = 0, 0, []
    for size, copied in want:
        off = (used + 255) & ~255
        used = off + size
        expect.append([str(off), str(size), "1" if copied else "-"])
    assert placed == expect
    for (o, s, _), (o2, _, _) in zip(placed, placed[1:]):
        assert int(o) % 256 == 0 and int(o2) % 256 == 0 and int(o) + int(s) <= int(o2)
    assert need == used and cap == capacity(T, Q)
    assert need <= cap and overflow == 0


def test_the_program_refuses_a_malformed_row(answers):
    for row in ("resolve:256:2000", "grid:", "plan:1", "stage:window:1:1:0", "stage:bow:1:1:0", "dead:50:zz", "arena:-1:0"):
        assert subprocess.run([EXE, row], capture_output=True, timeout=60).returncode == 2
