"""The local-BA graph's host plan (openvslam_amd/csrc/ba_graph_plan.inc) without a device: tests/ba_graph_plan_host.cc, built by the plain host
compiler from the plan alone, prints what the plan decides for the rows below. The expected values are written out by hand from the conditions
graph_create and solver_workspace_create of ba_graph.hip held before the plan was moved out of them, not generated from the plan: a landmark run
closes when its edges exceed 256 or it has 256 landmarks; a keyframe's edge list is cut into chunks of 512; the pairs (a, b >= a) a-major, their
rows dealt to eight XCDs in serpentine order; every array on the next 256-byte boundary, an empty one taking a byte. The index build is held to
a numpy restatement (a stable argsort by landmark and by keyframe). The GPU tests see the results of a whole optimisation only; a wrong partition
reads a neighbour's slots without failing, so what was decided is checked here."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
EXE = os.path.join(CPP, "ba_graph_plan_host")

MONO = np.dtype([("pose_idx", "<i4"), ("point_idx", "<i4"), ("obs_x", "<f8"), ("obs_y", "<f8"), ("inv_sigma_sq", "<f8")])
STEREO = np.dtype([("pose_idx", "<i4"), ("point_idx", "<i4"), ("obs_x", "<f8"), ("obs_y", "<f8"), ("obs_x_right", "<f8"), ("inv_sigma_sq", "<f8")])


def tri(n):
    return n * (n + 1) // 2


# ---- landmark partition: counts -> (pl_bound, wg_first[0 .. n_lm_wg])
LANDMARKS = [
    ("1x256", (256, [0, 256])),                       # 256 landmarks of one edge: one run
    ("1x257", (257, [0, 256, 257])),                  # the 257th opens the next
    ("128,128", (2 * tri(128), [0, 2])),              # 256 edges fit
    ("128,129", (tri(128) + tri(129), [0, 1, 2])),    # 257 do not
    ("255,1", (tri(255) + 1, [0, 2])),
    ("256,1", (tri(256) + 1, [0, 1, 2])),
    ("0,256,0,1", (tri(256) + 1, [0, 3, 4])),         # landmarks without edges ride along
    ("300,1x5", (tri(300) + 5, [0, 1, 6])),           # a landmark of 300 edges is a run of its own: first,
    ("1x3,300,1x3", (tri(300) + 6, [0, 3, 4, 7])),    # in the middle,
    ("1x5,300", (tri(300) + 5, [0, 5, 6])),           # last,
    ("300,300", (2 * tri(300), [0, 1, 2])),           # and next to another one
    ("0x300", (0, [0, 256, 300])),                    # no edge at all: the landmark count still closes the run
    ("0", (0, [0, 1])),                               # n_pt = 1
    ("5", (15, [0, 1])),
    ("270", (tri(270), [0, 1])),
]

# ---- keyframe chunks: counts -> (max_chunks, chunk_start[0 .. n_pose], chunk_kf)
CHUNKS = [
    ("0,1,512,513,1024", (9, [0, 0, 1, 2, 4, 6], [1, 2, 3, 3, 4, 4])),   # 0, 1, 1, 2, 2 chunks
    ("0", (1, [0, 0], [])),
    ("1", (1, [0, 1], [0])),                           # the bound n_edge / 512 + n_pose is tight
    ("513,513", (4, [0, 2, 4], [0, 0, 1, 1])),         # and here
    ("511,1", (3, [0, 1, 2], [0, 1])),
    ("1025", (3, [0, 3], [0, 0, 0])),
]

# ---- pair table and work order: n_free -> (n_pairs, capacity, fill of XCD 0 .. 7)
PAIRS = {
    0: (0, 1, [0] * 8),
    1: (1, 2, [1, 0, 0, 0, 0, 0, 0, 0]),
    2: (3, 3, [2, 1, 0, 0, 0, 0, 0, 0]),
    8: (36, 13, [8, 7, 6, 5, 4, 3, 2, 1]),
    9: (45, 15, [9, 8, 7, 6, 5, 4, 3, 3]),             # row 8 (one pair) goes to XCD 7: the serpentine turns round
    16: (136, 34, [17] * 8),                           # rows x and 15 - x: 16 - x + x + 1
    17: (153, 37, [20, 19, 19, 19, 19, 19, 19, 19]),   # row 16 turns round again: XCD 0
    48: (1176, 196, None),
}

# ---- graph arena: (n_pose, n_pt, n_edge, n_free) -> 21 offsets, (early, upload, dup_host, image, arena), (max_chunks, n_pairs, capacity)
GRAPH_ORDER = ("edges lm_start lm_edges lm_nmono pose_start pose_edges fixed active slot_of_pose pose_pt pair_ab slot_pose wg_pair lm_wg_first "
               "chunk_kf chunk_start lm_of_slot dup lm_tmp pose_part ledges").split()
GRAPHS = [
    # nothing but single bytes and a 432-byte pose_part: every array one 256-byte unit behind the last
    ((1, 1, 0, 0), ([256 * i for i in range(20)] + [5376], (256, 4096, 4096, 4352, 5632), (1, 0, 1))),
    ((3, 2, 1, 2), ([256 * i for i in range(20)] + [6400], (256, 4096, 4096, 4352, 6656), (3, 3, 3))),          # pose_part: 3 x 432 bytes
    ((4, 7, 10, 0), ([0] + [256 * i for i in range(2, 21)] + [6912], (512, 4352, 4352, 4608, 7424), (4, 0, 1))),   # 400 bytes of 40-byte records
    # config 5: 50 keyframes, 20 000 landmarks, 100 000 edges
    ((50, 20000, 100000, 48), ([0, 4000000, 4080128, 4480256, 4560384, 4560640, 4960768, 4961024, 5061120, 5061376, 5461504, 5470976, 5471232, 5477632,
                                5557760, 5558784, 5559040, 5959168, 5959424, 6599424, 6705408],
                               (4000000, 5559040, 5559040, 5559296, 10705408), (245, 1176, 196))),
]

# ---- solver arena: (n_pose, n_pt, n_edge, n_free, n_pairs, pl_bound, solve_doubles) -> 10 offsets, (arena, n_lists, ff_bytes, pl_ok)
SOLVER_ORDER = "hinv y s dxp scal fail edge_of pl_cnt pl_off pl_ent".split()
SOLVERS = [
    ((1, 1, 0, 0, 0, 0, 512), ([0, 256, 512, 4864, 5120, 5376, 5632, 5888, 6144, 6400], (6656, 0, 256, 1))),    # no edge: Y still takes a record
    ((3, 2, 1, 2, 3, 1, 512), ([0, 256, 512, 4864, 5120, 5376, 5632, 5888, 6144, 6400], (6656, 12, 256, 1))),
    ((50, 20000, 100000, 48, 1176, 400000, 87552), ([0, 1440000, 15840000, 16542976, 16545536, 16545792, 16546048, 20386048, 20404992, 20423936],
                                                    (23623936, 4704, 3840000, 1))),
    # the cap of the pair lists: 2^28 entries are stored, one more and pl_ent takes one entry
    ((2, 3, 4, 2, 3, 2 ** 28, 512), ([0, 256, 1024, 5376, 5632, 5888, 6144, 6400, 6656, 6912], (6912 + 8 * 2 ** 28, 12, 256, 1))),
    ((2, 3, 4, 2, 3, 2 ** 28 + 1, 512), ([0, 256, 1024, 5376, 5632, 5888, 6144, 6400, 6656, 6912], (7168, 12, 256, 0))),
]

# ---- slots: flags -> (slot, slot_pose)
SLOTS = [
    ("0110", ([0, -1, -1, 1], [0, 3])),
    ("1", ([-1], [])),                  # no free keyframe
    ("0", ([0], [0])),
    ("07", ([0, -1], [0])),             # any non-zero byte fixes a keyframe
    ("none:3", ([0, 1, 2], [0, 1, 2])),   # pose_fixed == NULL: all free
]


def edge_lists(seed=3, n_pose=7, n_pt=40, n_mono=230, n_stereo=170):
    """A shuffled edge list: landmarks with no edge, with mono only, stereo only and both; keyframe 5 observes nothing."""
    rng = np.random.default_rng(seed)
    mono, stereo = np.zeros(n_mono, MONO), np.zeros(n_stereo, STEREO)
    for e, lo in ((mono, 0), (stereo, 12)):
        e["pose_idx"] = rng.choice([0, 1, 2, 3, 4, 6], len(e))
        e["point_idx"] = rng.integers(lo, lo + 24, len(e))     # landmarks 0 .. 11 mono only, 12 .. 23 both, 24 .. 35 stereo only, 36 .. 39 unobserved
        for k in e.dtype.names[2:]:
            e[k] = rng.normal(size=len(e))
    return n_pose, n_pt, mono, stereo


def write_edges(path, n_pose, n_pt, mono, stereo):
    with open(path, "wb") as f:
        f.write(np.array([n_pose, n_pt, len(mono), len(stereo)], "<i4").tobytes())
        f.write(mono.tobytes())
        f.write(stereo.tobytes())
    return "index:" + str(path)


def bad_cases():
    """name -> (n_pose, n_pt, mono, stereo, the edge the parent's first pass stops at)"""
    out = {}
    n_pose, n_pt, mono, stereo = edge_lists()
    m = mono.copy()
    m["point_idx"][17] = n_pt                      # equal to n_pt, in the mono list; a later one is not reached
    m["pose_idx"][40] = n_pose
    out["mono_pt"] = (n_pose, n_pt, m, stereo, 17)
    m = mono.copy()
    m["pose_idx"][len(m) - 1] = n_pose             # equal to n_pose, the last mono edge
    out["mono_pose"] = (n_pose, n_pt, m, stereo, len(m) - 1)
    m = mono.copy()
    m["pose_idx"][0] = -1                          # negative, the first edge
    out["negative"] = (n_pose, n_pt, m, stereo, 0)
    s = stereo.copy()
    s["point_idx"][5] = -3                         # in the stereo list: stereo edges count from n_mono
    s["point_idx"][4] = n_pt - 1                   # (the largest valid index just before it)
    out["stereo_pt"] = (n_pose, n_pt, mono, s, len(mono) + 5)
    s = stereo.copy()
    s["pose_idx"][len(s) - 1] = n_pose + 100
    out["stereo_pose"] = (n_pose, n_pt, mono, s, len(mono) + len(s) - 1)
    m, s = mono.copy(), stereo.copy()
    m["point_idx"][200] = 2 ** 31 - 1              # a bad mono edge is found before a bad stereo edge
    s["pose_idx"][0] = n_pose
    out["mono_first"] = (n_pose, n_pt, m, s, 200)
    return out


def all_rows(tmp):
    """Every row of the tables above -> its argument for the program (the edge lists are written into tmp)."""
    rows = {("lm", c): "lm:" + c for c, _ in LANDMARKS}
    rows.update({("chunks", c): "chunks:" + c for c, _ in CHUNKS})
    rows.update({("pairs", n): "pairs:%d" % n for n in list(PAIRS) + list(range(3, 41))})
    rows.update({("slots", f): "slots:" + f for f, _ in SLOTS})
    rows.update({("graph", r): "graph:%d:%d:%d:%d" % r for r, _ in GRAPHS})
    rows.update({("solver", r): "solver:%d:%d:%d:%d:%d:%d:%d" % r for r, _ in SOLVERS})
    rows[("index", "good")] = write_edges(os.path.join(tmp, "good.bin"), *edge_lists())
    n_pose, n_pt, mono, stereo = edge_lists()
    rows[("index", "mono_only")] = write_edges(os.path.join(tmp, "mono_only.bin"), n_pose, n_pt, mono, stereo[:0])
    rows[("index", "stereo_only")] = write_edges(os.path.join(tmp, "stereo_only.bin"), n_pose, n_pt, mono[:0], stereo)
    rows[("index", "empty")] = write_edges(os.path.join(tmp, "empty.bin"), 1, 1, mono[:0], stereo[:0])
    for name, case in bad_cases().items():
        rows[("index", name)] = write_edges(os.path.join(tmp, name + ".bin"), *case[:4])
    return rows


def run_rows(exe, rows):
    keys = list(rows)
    r = subprocess.run([exe] + [rows[k] for k in keys], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(keys)
    return dict(zip(keys, lines))


def ints(line):
    return [[int(v) for v in part.split()] for part in line.split("|")]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", CPP, "ba_graph_plan_host"])
    return run_rows(EXE, all_rows(str(tmp_path_factory.mktemp("ba_graph_plan"))))


@pytest.mark.parametrize("counts,want", LANDMARKS, ids=[c for c, _ in LANDMARKS])
def test_landmark_partition(answers, counts, want):
    (n_wg, pl_bound), first = ints(answers[("lm", counts)])
    assert (pl_bound, first) == want and n_wg == len(first) - 1
    # whole landmarks, at most 256 edges and 256 landmarks; a run above 256 edges is one landmark; the runs tile [0, n_pt)
    n = []
    for part in counts.split(","):
        c, _, rep = part.partition("x")
        n += [int(c)] * int(rep or 1)
    assert first[0] == 0 and first[-1] == len(n) and all(a < b for a, b in zip(first, first[1:]))
    for a, b in zip(first, first[1:]):
        assert b - a <= 256 and (sum(n[a:b]) <= 256 or b - a == 1)
    assert pl_bound == sum(tri(c) for c in n)


@pytest.mark.parametrize("counts,want", CHUNKS, ids=[c for c, _ in CHUNKS])
def test_keyframe_chunks(answers, counts, want):
    (n_chunks, max_chunks), start, kf = ints(answers[("chunks", counts)])
    assert (max_chunks, start, kf) == want
    assert start[-1] == n_chunks == len(kf) <= max_chunks


@pytest.mark.parametrize("n_free", sorted(PAIRS) + list(range(3, 41)))
def test_pair_table_and_work_order(answers, n_free):
    (n_pairs, cap, n_pair_wg), pair_ab, wg_pair = ints(answers[("pairs", n_free)])
    assert n_pairs == tri(n_free) and cap == n_pairs // 8 + n_free + 1
    assert pair_ab == [v for a in range(n_free) for b in range(a, n_free) for v in (a, b)]     # a-major
    if n_free == 0:
        assert n_pair_wg == 0 and wg_pair == []      # nothing is written (the program passed null pointers)
        return
    assert len(wg_pair) == 8 * cap
    seq = [[p for p in wg_pair[x::8]] for x in range(8)]     # workgroup 8 i + x belongs to XCD x
    fill = [sum(p >= 0 for p in s) for s in seq]
    if n_free in PAIRS:
        want_pairs, want_cap, want_fill = PAIRS[n_free]
        assert (n_pairs, cap) == (want_pairs, want_cap) and (want_fill is None or fill == want_fill)
    assert n_pair_wg == 8 * max(fill) and max(fill) <= cap
    assert sorted(p for p in wg_pair if p >= 0) == list(range(n_pairs))     # every pair exactly once
    first = [a * n_free - a * (a - 1) // 2 for a in range(n_free)]          # index of pair (a, a)
    for x, s in enumerate(seq):
        assert all(p == -1 for p in s[fill[x]:])     # everything else is -1, and a sequence has no hole
        rows = [a for a in range(n_free) if (7 - a % 8 if (a // 8) % 2 else a % 8) == x]     # serpentine: rows 0 .. 7 up, 8 .. 15 down, ...
        assert s[:fill[x]] == [first[a] + i for a in rows for i in range(n_free - a)]         # whole rows, each contiguous, in row order


@pytest.mark.parametrize("flags,want", SLOTS, ids=[f for f, _ in SLOTS])
def test_free_keyframe_slots(answers, flags, want):
    (n_free,), slot, slot_pose = ints(answers[("slots", flags)])
    assert (slot, slot_pose) == want and n_free == len(slot_pose)


@pytest.mark.parametrize("row,want", GRAPHS, ids=["%d_%d_%d_%d" % r for r, _ in GRAPHS])
def test_graph_arena(answers, row, want):
    off, (early, upload, dup_host, image, arena), counts = ints(answers[("graph", row)])
    assert (off, (early, upload, dup_host, image, arena), tuple(counts)) == want
    n_pose, n_pt, ne, nf = row
    max_chunks, n_pairs, cap = counts
    assert (max_chunks, n_pairs, cap) == (ne // 512 + n_pose, tri(nf), tri(nf) // 8 + nf + 1)
    o = dict(zip(GRAPH_ORDER, off))
    assert all(v % 256 == 0 for v in off) and all(a < b for a, b in zip(off, off[1:]))     # aligned, strictly ascending in the documented order
    size = {"edges": 40 * ne, "lm_start": 4 * (n_pt + 1), "lm_edges": 4 * ne, "lm_nmono": 4 * n_pt, "pose_start": 4 * (n_pose + 1), "pose_edges": 4 * ne,
            "fixed": n_pose, "active": ne, "slot_of_pose": 4 * n_pose, "pose_pt": 4 * ne, "pair_ab": 8 * n_pairs, "slot_pose": 4 * nf,
            "wg_pair": 32 * cap, "lm_wg_first": 4 * (n_pt + 1), "chunk_kf": 4 * max_chunks, "chunk_start": 4 * (n_pose + 1), "lm_of_slot": 4 * ne,
            "dup": 8, "lm_tmp": 32 * n_pt, "pose_part": 8 * 27 * 2 * max_chunks, "ledges": 40 * ne}
    for name, nxt in zip(GRAPH_ORDER, off[1:] + [arena]):
        assert o[name] + size[name] <= nxt, name     # no array reaches into the next
    assert early == o["lm_start"]                                    # the early upload is the records
    assert o["chunk_start"] + size["chunk_start"] <= upload == o["lm_of_slot"]   # the upload ends before what the device writes
    assert dup_host == upload and image == upload + 256              # the image: the upload and the verdict's word
    assert arena % 256 == 0 and image % 256 == 0


@pytest.mark.parametrize("row,want", SOLVERS, ids=["%d_%d_%d_%d_%d_%d_%d" % r for r, _ in SOLVERS])
def test_solver_arena(answers, row, want):
    off, (arena, n_lists, ff_bytes, pl_ok) = ints(answers[("solver", row)])
    assert (off, (arena, n_lists, ff_bytes, pl_ok)) == want
    n_pose, n_pt, ne, nf, n_pairs, pl_bound, solve_doubles = row
    o = dict(zip(SOLVER_ORDER, off))
    assert all(v % 256 == 0 for v in off) and all(a < b for a, b in zip(off, off[1:]))
    assert pl_ok == (pl_bound <= 2 ** 28) and n_lists == 4 * n_pairs
    size = {"hinv": 72 * n_pt, "y": 144 * max(ne, 1), "s": 8 * (solve_doubles + 6 * n_pose), "dxp": 48 * n_pose, "scal": 256, "fail": 8,
            "edge_of": 4 * max(nf, 1) * n_pt, "pl_cnt": 4 * (n_lists + 1), "pl_off": 4 * (n_lists + 1), "pl_ent": 8 * (max(pl_bound, 1) if pl_ok else 1)}
    for name, nxt in zip(SOLVER_ORDER, off[1:] + [arena]):
        assert o[name] + size[name] <= nxt, name
    assert o["fail"] - o["scal"] == 256                  # one download takes d_scal and both failure words (ba_optimize.hip's TrialBlock)
    assert o["edge_of"] + ff_bytes == o["pl_cnt"]        # the 0xff memset: the table and its padding, nothing of pl_cnt


def restate(n_pose, n_pt, mono, stereo):
    """The index build in numpy: counting sorts = stable argsorts by landmark and by keyframe."""
    pose = np.concatenate([mono["pose_idx"], stereo["pose_idx"]]).astype(np.int64)
    pt = np.concatenate([mono["point_idx"], stereo["point_idx"]]).astype(np.int64)
    lm_edges, pose_edges = np.argsort(pt, kind="stable"), np.argsort(pose, kind="stable")
    return {"lm_start": np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=n_pt))]), "lm_edges": lm_edges,
            "lm_nmono": np.bincount(mono["point_idx"], minlength=n_pt), "pose_start": np.concatenate([[0], np.cumsum(np.bincount(pose, minlength=n_pose))]),
            "pose_edges": pose_edges, "pose_pt": pt[pose_edges], "pose": pose, "pt": pt}


@pytest.mark.parametrize("case", ["good", "mono_only", "stereo_only", "empty"])
def test_index_build_matches_a_stable_argsort(answers, case):
    n_pose, n_pt, mono, stereo = edge_lists()
    if case == "mono_only":
        stereo = stereo[:0]
    elif case == "stereo_only":
        mono = mono[:0]
    elif case == "empty":
        n_pose, n_pt, mono, stereo = 1, 1, mono[:0], stereo[:0]
    parts = answers[("index", case)].split("|")
    assert parts[0].strip() == "ok" and len(parts) == 9
    got = dict(zip(("lm_start", "lm_edges", "lm_nmono", "pose_start", "pose_edges", "pose_pt"), ([int(v) for v in p.split()] for p in parts[1:7])))
    want = restate(n_pose, n_pt, mono, stereo)
    for k, v in got.items():
        assert v == want[k].tolist(), k
    n_mono, ne = len(mono), len(mono) + len(stereo)
    # within a landmark the edges ascend, so mono (the lower indices) comes before stereo, lm_nmono of them
    for j in range(n_pt):
        mine = got["lm_edges"][got["lm_start"][j]:got["lm_start"][j + 1]]
        assert mine == sorted(mine) and sum(e < n_mono for e in mine) == got["lm_nmono"][j]
        assert all(e < n_mono for e in mine[:got["lm_nmono"][j]])
    for k in range(n_pose):
        mine = got["pose_edges"][got["pose_start"][k]:got["pose_start"][k + 1]]
        assert mine == sorted(mine)
    assert got["pose_pt"] == [int(want["pt"][e]) for e in got["pose_edges"]]
    # the records: mono then stereo, a mono edge's right coordinate 0
    ids = [int(v) for v in parts[7].split()]
    assert ids == [int(v) for e in range(ne) for v in (want["pose"][e], want["pt"][e])]
    vals = [float.fromhex(v) for v in parts[8].split()]
    rec = [(e["obs_x"], e["obs_y"], 0.0, e["inv_sigma_sq"]) for e in mono] + [(e["obs_x"], e["obs_y"], e["obs_x_right"], e["inv_sigma_sq"]) for e in stereo]
    assert vals == [float(v) for r in rec for v in r]


@pytest.mark.parametrize("case", sorted(bad_cases()))
def test_index_build_reports_the_first_bad_edge(answers, case):
    assert answers[("index", case)] == "bad %d" % bad_cases()[case][4]


def test_the_program_refuses_a_malformed_row(answers):
    for row in ("lm:", "lm:1x", "chunks:-1", "pairs:x", "graph:1:1:0", "solver:1", "slots:", "index:/nonexistent", "plan:1"):
        assert subprocess.run([EXE, row], capture_output=True, timeout=60).returncode == 2, row


def test_host_program_runs_clean_under_the_sanitizers(answers, tmp_path):
    """The same rows through the same program built with AddressSanitizer and UndefinedBehaviorSanitizer; the program sizes every array as the
    plan does, so a write past a partition's or a sort's array stops it. It stands alone: the runtimes are inside it."""
    exe = str(tmp_path / "ba_graph_plan_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "openvslam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "ba_graph_plan_host.cc")])
    rows = all_rows(str(tmp_path))
    got = run_rows(exe, rows)
    assert len(got) == len(answers) and all(got[k] == answers[k] for k in answers)
