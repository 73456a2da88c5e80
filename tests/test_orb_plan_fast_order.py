"""k_fast_cells' work order without a device. The kernel finds its (frame, group) from the workgroup index with a multiply-high by a host-built
magic instead of a division (openvslam_amd/csrc/fast_order.inc, compiled into the kernel, into launch_fast and, here, into tests/fast_order_host.cc
by the plain host compiler). Held to the plain division for EVERY gid of representative launches, the largest admitted ones included, and at
the edges of the whole 32-bit range; the clipped-cell pixel mask, which moved into the same file, is held to its definition exhaustively."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvslam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fast_order") / "fast_order_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "fast_order_host.cc")])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (args, r.returncode, r.stderr)
    return [int(v) for v in r.stdout.split()]


def admitted(n_cells, batch):
    """launch_fast's bound, restated: ceil(n_cells / 8) * batch^2 < 2^32, and a grid that fits 32 bits"""
    return -(-n_cells // 8) * batch * batch < 2 ** 32 and (n_cells + 7) * batch < 2 ** 32


# (n_cells, cells_per_wg, batch): n_groups of 1, 2, 3, 7, 8, 9 and 523 (the 1 568 cells of 1080p in threes), groups that do not divide the cells,
# more cells per group than cells, the bench's launch, and the largest launches the bound admits: most frames (8 cells), most cells of a
# geometry (sides <= 8191: below 2^16) with the most frames those allow, and 2^26 groups of one frame (a thousand times any geometry's)
ORDER_CASES = [(1, 3, 1), (1, 1, 5), (2, 1, 3), (9, 3, 1), (9, 3, 9), (7, 1, 4), (8, 1, 4), (8, 1, 1), (9, 1, 3), (9, 1, 8), (1568, 3, 1), (1568, 3, 3), (1568, 3, 256),
               (1568, 2, 64), (1568, 64, 9), (87, 100, 7), (87, 2, 9), (20, 3, 9),
               (8, 1, 65535), (65535, 1, 724), (65535, 3, 724), (2 ** 26, 1, 1)]
REFUSED = [(8, 65536), (65535, 725), (9, 46341), (2 ** 31 - 1, 3), (2 ** 31 - 1, 2)]


@pytest.mark.parametrize("case", ORDER_CASES, ids=lambda c: "%dx%dx%d" % c)
def test_magic_work_order_equals_the_division_for_every_gid(exe, case):
    n_cells, cpw, batch = case
    assert admitted(n_cells, batch)
    n_groups = -(-n_cells // cpw)
    total = n_groups * batch
    ok, got_groups, share, got_total, grid, covered, bad_frame, bad_group, bad_gid = run(exe, "order", n_cells, cpw, batch)
    assert ok == 1
    assert (got_groups, got_total, share) == (n_groups, total, -(-total // 8))
    assert grid == 8 * -(-n_groups // 8) * batch and grid >= 8 * share   # every XCD's share has its workgroups
    assert covered == total                                              # every (frame, group) is worked on exactly once
    assert (bad_frame, bad_group, bad_gid) == (0, 0, 0)


def test_the_cases_reach_the_group_counts_the_order_turns_on():
    assert {-(-n // c) for n, c, _ in ORDER_CASES} >= {1, 2, 3, 7, 8, 9, 523}
    assert any(-(-n // 8) * (b + 1) ** 2 >= 2 ** 32 for n, _, b in ORDER_CASES)   # a launch with one frame more would be refused


@pytest.mark.parametrize("n_cells,batch", REFUSED)
def test_launches_beyond_the_bound_are_refused(exe, n_cells, batch):
    assert not admitted(n_cells, batch)
    assert run(exe, "order", n_cells, 1, batch) == [0]


def test_magic_quotient_is_exact_at_the_edges_of_the_32_bit_range(exe):
    divisors = [1, 2, 3, 7, 8, 9, 523, 641, 65535, 65536, 65537, 6700417, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1]
    checked, bad = run(exe, "magic", *divisors)
    assert checked > 200000 * 3 and bad == 0


def test_clipped_cell_mask_equals_its_definition(exe):
    checked, bad = run(exe, "mask")
    assert checked == 8 * 32 * 73 * 73 and bad == 0
