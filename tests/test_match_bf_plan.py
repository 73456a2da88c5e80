"""The brute-force matcher's host plan (openvslam_amd/csrc/match_bf_plan.inc) without a device: tests/match_bf_plan_host.cc, built by the plain host
compiler from the plan alone, prints what the plan decides for the rows below. The expected values are written out by hand from the conditions
match_hamming.hip held before the plan was moved out of it (near_threshold, the sizes and the two comparisons of ovs_matcher_create, run_bf's launch
geometry, the pointer arithmetic at the head of k_bf_resolve and the first lines of the four entry points), not generated from the plan. The GPU tests
see results only; which form of the resolver a handle runs is visible here."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
EXE = os.path.join(CPP, "match_bf_plan_host")
KIB = 1024
OK, INVALID, CAPACITY, ALIGN = 0, -1, -4, -5


def fhex(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


def round16(x):
    return (x + 15) & ~15


# ---- resolver: (max_n1, max_n2) -> (refused, staged, waves, block, dynamic LDS bytes, attribute raised) -----------------------------------------
# one wave: 4 n1 + round16(n1) bytes, refused above 150 KiB; staged (four waves) while round16(5 n1) + 36 n2 <= 150 KiB; the attribute above 64 KiB
REFUSED = (1, 0, 0, 0, 0, 0)
RESOLVE = [
    ((1, 1), (0, 1, 4, 256, 52, 0)),
    ((128, 128), (0, 1, 4, 256, 5248, 0)),
    ((256, 256), (0, 1, 4, 256, 10496, 0)),
    ((1560, 1560), (0, 1, 4, 256, 63968, 0)),
    ((1587, 1600), (0, 1, 4, 256, 65536, 0)),             # round16(7935) + 57600 = 64 KiB exactly: the last without the attribute
    ((1588, 1600), (0, 1, 4, 256, 65552, 1)),             # round16(7940) = 7952
    ((1587, 1601), (0, 1, 4, 256, 65572, 1)),
    ((2048, 2048), (0, 1, 4, 256, 83968, 1)),             # the benchmark's handle
    ((3000, 3000), (0, 1, 4, 256, 123008, 1)),
    ((2048, 3982), (0, 1, 4, 256, 153592, 1)),            # 10240 + 143352
    ((2048, 3983), (0, 0, 1, 64, 10240, 0)),              # 10240 + 143388 > 150 KiB
    ((2048, 4096), (0, 0, 1, 64, 10240, 0)),              # the one-wave handle of tests/test_gpu_match.py
    ((3746, 3746), (0, 1, 4, 256, 153592, 1)),            # the last square size that stages
    ((3747, 3747), (0, 0, 1, 64, 18748, 0)),
    ((4096, 4096), (0, 0, 1, 64, 20480, 0)),              # the class layer's handle (cpp/openvslam/match/robust.cc)
    ((13104, 4096), (0, 0, 1, 64, 65520, 0)),             # 52416 + 13104: the last one-wave size without the attribute
    ((13105, 4096), (0, 0, 1, 64, 65540, 1)),             # 52420 + 13120
    ((16384, 2048), (0, 0, 1, 64, 81920, 1)),
    ((16384, 1), (0, 1, 4, 256, 81956, 1)),
    ((30710, 1), (0, 1, 4, 256, 153588, 1)),              # round16(153550) + 36: the longest frame side that stages
    ((30711, 1), (0, 0, 1, 64, 153564, 1)),               # round16(153555) + 36 = 153604; one wave: 122844 + 30720
    ((30720, 1), (0, 0, 1, 64, 153600, 1)),               # the last size accepted
    ((30721, 1), REFUSED),
    ((65535, 1), REFUSED),
    ((1, 65535), (0, 0, 1, 64, 20, 0)),
    ((1, 4266), (0, 1, 4, 256, 153592, 1)),               # 16 + 153576
    ((1, 4267), (0, 0, 1, 64, 20, 0)),
]

# ---- near_threshold: max(50, tau - 1) capped at 255, tau the smallest s in 0 .. 256 with !(fl(ratio * s) < 50), 257 if there is none -------------
NEAR_THR = [
    (0.6, 83), (0.75, 66), (0.9, 55), (1.0, 50), (1.01, 50), (0.1, 255), (0.0, 255), (float("nan"), 255),   # NaN: tau = 0, tau - 1 wraps around
    (-0.8, 255), (float("inf"), 255),   # inf: fl(inf * 0) is NaN at s = 0, the same wrap-around
    (0.5, 99), (50.0 / 256.0, 255), (0.2, 249), (2.0, 50), (50.0, 50), (51.0, 50),
]

# ---- near launch: (max_n2, batch, path) -> (chunks, total_wg, grid); 256 queries per workgroup (matrix, 0), 64 (popcount, 1); grid on 8 -----------
NEAR = [
    ((2048, 128, 0), (8, 1024, 1024)), ((2048, 1, 0), (8, 8, 8)), ((300, 3, 0), (2, 6, 8)), ((300, 3, 1), (5, 15, 16)),
    ((1, 1, 0), (1, 1, 8)), ((1, 1, 1), (1, 1, 8)), ((256, 1, 0), (1, 1, 8)), ((257, 1, 0), (2, 2, 8)), ((64, 9, 1), (1, 9, 16)), ((65, 8, 1), (2, 16, 16)),
    ((4096, 1, 0), (16, 16, 16)), ((4096, 1, 1), (64, 64, 64)), ((65535, 1, 0), (256, 256, 256)),
]

# ---- buffers: (max_n1, max_n2, max_batch) -> the thirteen hipMalloc sizes of ovs_matcher_create, in its order -------------------------------------
BUFFERS = [(128, 128, 1), (2048, 2048, 128), (4096, 4096, 1), (100, 200, 3), (200, 100, 3), (65535, 1, 1), (1, 65535, 2)]


def buffers(n1, n2, B):
    return (4 * B * n2 * 4, 4 * B * n2 * 4 * 64, 4 * B * n2 * 8, n1 * 32, n2 * 32, max(n1, n2), n1, 8, 8 * n2, 4, 4 * n2, 2 * n2, 2 * n2)


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
# ovs_matcher_create(out, max_n1, max_n2, max_batch): INVALID before CAPACITY
CREATE = [
    ((1, 128, 128, 1), OK), ((1, 4096, 4096, 1), OK), ((1, 65535, 1, 1), CAPACITY), ((1, 30720, 1, 1), OK), ((1, 30721, 1, 1), CAPACITY),
    ((0, 128, 128, 1), INVALID), ((1, 0, 128, 1), INVALID), ((1, 128, 0, 1), INVALID), ((1, 128, 128, 0), INVALID), ((1, 65536, 1, 1), INVALID),
    ((1, 1, 65536, 1), INVALID), ((1, 65536, 65536, 1), INVALID), ((1, 30721, 1, 0), INVALID), ((0, 30721, 1, 1), INVALID), ((1, 30721, 65536, 1), INVALID),
    ((1, -1, 1, 1), INVALID),
]
# ovs_robust_brute_force_match on a 100 x 200 handle: (handle, desc_1, n1, desc_2, n2, pairs, cap, n_out) -> (status, runs, *n_out; 7 = not written)
MATCH = [
    ((1, 1, 100, 1, 200, 1, 200, 1), (OK, 1, 0)),
    ((1, 1, 100, 1, 200, 0, 0, 1), (OK, 1, 0)),                 # cap == 0 needs no pairs
    ((1, 1, 100, 1, 200, 0, 1, 1), (INVALID, 0, 0)),
    ((0, 1, 100, 1, 200, 1, 200, 1), (INVALID, 0, 7)),
    ((1, 1, 100, 1, 200, 1, 200, 0), (INVALID, 0, 7)),
    ((1, 1, -1, 1, 200, 1, 200, 1), (INVALID, 0, 7)),
    ((1, 1, 100, 1, -1, 1, 200, 1), (INVALID, 0, 7)),
    ((1, 1, 100, 1, 200, 1, -1, 1), (INVALID, 0, 7)),
    ((1, 0, 0, 0, 200, 0, 5, 1), (OK, 0, 0)),                   # n1 == 0: done, whatever the pointers
    ((1, 0, 100, 0, 0, 0, 5, 1), (OK, 0, 0)),
    ((1, 0, 0, 1, 201, 1, 5, 1), (OK, 0, 0)),                   # ... and before the capacity is looked at
    ((1, 0, 100, 1, 200, 1, 200, 1), (INVALID, 0, 0)),
    ((1, 1, 100, 0, 200, 1, 200, 1), (INVALID, 0, 0)),
    ((1, 1, 101, 1, 200, 1, 200, 1), (CAPACITY, 0, 0)),
    ((1, 1, 100, 1, 201, 1, 200, 1), (CAPACITY, 0, 0)),
    ((1, 0, 101, 1, 200, 1, 200, 1), (INVALID, 0, 0)),          # INVALID before CAPACITY
    ((1, 1, 1, 1, 1, 1, 1, 1), (OK, 1, 0)),
]
# ovs_robust_brute_force_match_batch_dev on a 100 x 200 x 4 handle: (handle, all pointers set, desc_1, stride_1, desc_2, stride_2, batch, cap)
BATCH = [
    ((1, 1, 4096, 3200, 8192, 6400, 4, 200), OK),
    ((1, 1, 4096, 32, 8192, 32, 1, 1), OK),
    ((1, 1, 4096, 0, 8192, 0, 1, 1), OK),                       # stride 0: every problem the same block (the parent accepted it)
    ((0, 1, 4096, 3200, 8192, 6400, 4, 200), INVALID),
    ((1, 0, 4096, 3200, 8192, 6400, 4, 200), INVALID),
    ((1, 1, 4096, 3200, 8192, 6400, 0, 200), INVALID),
    ((1, 1, 4096, 3200, 8192, 6400, 4, 0), INVALID),
    ((1, 1, 4096, 3200, 8192, 6400, 5, 200), CAPACITY),
    ((1, 1, 4096, 3232, 8192, 6400, 4, 200), CAPACITY),
    ((1, 1, 4096, 3200, 8192, 6432, 4, 200), CAPACITY),
    ((1, 1, 4097, 3200, 8192, 6400, 4, 200), ALIGN),
    ((1, 1, 4096, 3200, 8194, 6400, 4, 200), ALIGN),
    ((1, 1, 4096, 3184, 8192, 6400, 4, 200), ALIGN),
    ((1, 1, 4096, 3200, 8192, 6399, 4, 200), ALIGN),
    ((1, 1, 4097, 3201, 8192, 6400, 4, 200), CAPACITY),         # CAPACITY before ALIGN
    ((1, 1, 4097, 3200, 8192, 6400, 5, 0), INVALID),            # INVALID before both
]
# ovs_hamming_best2 on a 100 x 200 handle (targets ride in the idx_1 buffers, queries in the idx_2 buffers): (handle, q, nq, t, nt, outputs)
BEST2 = [
    ((1, 1, 200, 1, 100, 1), (OK, 1)),
    ((1, 1, 200, 0, 0, 1), (OK, 1)),                            # no targets: t may be NULL
    ((1, 1, 200, 0, 1, 1), (INVALID, 0)),
    ((0, 1, 200, 1, 100, 1), (INVALID, 0)),
    ((1, 1, -1, 1, 100, 1), (INVALID, 0)),
    ((1, 1, 200, 1, -1, 1), (INVALID, 0)),
    ((1, 0, 0, 0, 101, 0), (OK, 0)),                            # nq == 0: done, whatever the rest
    ((1, 0, 200, 1, 100, 1), (INVALID, 0)),
    ((1, 1, 200, 1, 100, 0), (INVALID, 0)),
    ((1, 1, 201, 1, 100, 1), (CAPACITY, 0)),
    ((1, 1, 200, 1, 101, 1), (CAPACITY, 0)),
    ((1, 0, 201, 1, 100, 1), (INVALID, 0)),                     # INVALID before CAPACITY
]


def all_rows():
    return (["consts"] + ["thr:%s" % fhex(r) for r, _ in NEAR_THR] + ["resolve:%d:%d" % k for k, _ in RESOLVE] + ["near:%d:%d:%d" % k for k, _ in NEAR]
            + ["buffers:%d:%d:%d" % k for k in BUFFERS] + ["create:%d:%d:%d:%d" % k for k, _ in CREATE] + ["match:%d:100:200:%d:%d:%d:%d:%d:%d:%d" % k for k, _ in MATCH]
            + ["batch:%d:100:200:4:%d:%d:%d:%d:%d:%d:%d" % k for k, _ in BATCH] + ["best2:%d:100:200:%d:%d:%d:%d:%d" % k for k, _ in BEST2])


def run_rows(exe, rows):
    r = subprocess.run([exe] + rows, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    return {row: tuple(int(v) for v in line.split()) for row, line in zip(rows, lines)}


@pytest.fixture(scope="module")
def answers():
    subprocess.check_call(["make", "-s", "-C", CPP, "match_bf_plan_host"])
    return run_rows(EXE, all_rows())


def test_shared_constants(answers):
    """kNearSplit, kNearSeg, kTopK, kNearQueries and the popcount form's queries per workgroup: what the kernels' static_asserts and layouts rest on."""
    assert answers["consts"] == (4, 64, 8, 256, 64)


@pytest.mark.parametrize("ratio,want", NEAR_THR, ids=["r%s" % r for r, _ in NEAR_THR])
def test_near_threshold(answers, ratio, want):
    assert answers["thr:%s" % fhex(ratio)] == (want,)


@pytest.mark.parametrize("key,want", RESOLVE, ids=["n%d_m%d" % k for k, _ in RESOLVE])
def test_resolver_plan(answers, key, want):
    assert answers["resolve:%d:%d" % key][:6] == want


@pytest.mark.parametrize("key", [k for k, _ in RESOLVE], ids=["n%d_m%d" % k for k, _ in RESOLVE])
def test_resolver_lds_layout(answers, key):
    """The layout as k_bf_resolve's pointer arithmetic stated it: mark u32[n1] at 0, claimed u8[n1] behind it, the top-8 table u32[n2][8] on the next
    16 bytes, the packed counts u32[n2] behind that. Sections disjoint and in bounds of what the plan asks for: all four in the staged form, mark and
    claimed in the one-wave form (which never touches the other two)."""
    n1, n2 = key
    refused, staged, _, _, lds_bytes, _, mark, claimed, tops, cnts, total = answers["resolve:%d:%d" % key]
    assert (mark, claimed, tops, cnts, total) == (0, 4 * n1, round16(5 * n1), round16(5 * n1) + 32 * n2, round16(5 * n1) + 36 * n2)
    sections = [(mark, 4 * n1), (claimed, n1), (tops, 32 * n2), (cnts, 4 * n2)]
    for (o, s), (o2, _) in zip(sections, sections[1:]):
        assert o + s <= o2
    assert mark % 4 == 0 and tops % 16 == 0 and cnts % 4 == 0
    if refused:
        assert 4 * n1 + round16(n1) > 150 * KIB
        return
    assert lds_bytes <= 150 * KIB
    if staged:
        assert cnts + 4 * n2 <= lds_bytes == total
    else:
        assert claimed + n1 <= lds_bytes == 4 * n1 + round16(n1) and total > 150 * KIB


@pytest.mark.parametrize("key,want", NEAR, ids=["m%d_b%d_p%d" % k for k, _ in NEAR])
def test_near_launch(answers, key, want):
    got = answers["near:%d:%d:%d" % key]
    assert got == want
    chunks, total_wg, grid = got
    per_wg = 64 if key[2] else 256
    assert chunks * per_wg >= key[0] > (chunks - 1) * per_wg and grid % 8 == 0 and 0 <= grid - total_wg < 8


@pytest.mark.parametrize("key", BUFFERS, ids=["n%d_m%d_b%d" % k for k in BUFFERS])
def test_buffer_sizes(answers, key):
    assert answers["buffers:%d:%d:%d" % key] == buffers(*key)


def test_argument_checks_of_create(answers):
    for k, want in CREATE:
        assert answers["create:%d:%d:%d:%d" % k] == (want,), k


def test_argument_checks_of_brute_force_match(answers):
    for k, want in MATCH:
        assert answers["match:%d:100:200:%d:%d:%d:%d:%d:%d:%d" % k] == want, k


def test_argument_checks_of_batch_dev(answers):
    for k, want in BATCH:
        assert answers["batch:%d:100:200:4:%d:%d:%d:%d:%d:%d:%d" % k] == (want,), k


def test_argument_checks_of_best2(answers):
    for k, want in BEST2:
        assert answers["best2:%d:100:200:%d:%d:%d:%d:%d" % k] == want, k


def test_the_program_refuses_a_malformed_row(answers):
    for row in ("resolve:256", "resolve:0:1", "thr:zz", "near:1:1", "buffers:0:1:1", "plan:1", "create:1:1:1", "match:1", "best2:", "consts:1"):
        assert subprocess.run([EXE, row], capture_output=True, timeout=60).returncode == 2, row


def test_host_program_runs_clean_under_the_sanitizers(answers):
    """A stand-alone program with its own main on this CPU, AddressSanitizer and UndefinedBehaviorSanitizer linked in: the same rows, the same
    answers. The test puts nothing into the child's environment and takes nothing out of it."""
    subprocess.check_call(["make", "-s", "-C", CPP, "match_bf_plan_host_san"])
    assert run_rows(os.path.join(CPP, "match_bf_plan_host_san"), all_rows()) == answers
