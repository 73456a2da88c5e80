"""The pose optimiser's launch plan (openvslam_amd/csrc/pose_plan.inc) without a device: tests/pose_plan_host.cc, built by the plain host compiler
from the plan alone, prints what the plan decides for the rows below. The expected values are written out by hand from the conditions the two
host functions of pose_opt.hip held before the plan was moved out of them (workgroups from 500 / 850 / 1600 observations, 512 threads from
768 / 1500 in one workgroup, records in registers up to 2 * groups * 256, batched retries on several workgroups or up to 512 observations), not
generated from the plan. The GPU tests see results only; which form ran is visible here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")


def frame(n, model=0, threads=0, groups=0, retries=-1, obs_regs=1, zero_copy=1, first=1):
    return "frame:%d:%d:%d:%d:%d:%d:%d:%d" % (model, n, threads, groups, retries, obs_regs, zero_copy, first)


def batch(threads=0, groups=0, retries=-1, obs_regs=1, zero_copy=1):
    return "batch:%d:%d:%d:%d:%d" % (threads, groups, retries, obs_regs, zero_copy)


# row -> (threads, groups, batch_retries, kreg, zero_copy)
LAUNCHES = [
    # default switches, perspective: 1 / 2 / 4 / 8 workgroups, records in registers and read from the pinned block up to 2 * groups * 256
    (frame(4), (256, 1, 1, 2, 1)),
    (frame(5), (256, 1, 1, 2, 1)),
    (frame(499), (256, 1, 1, 2, 1)),
    (frame(500), (256, 2, 1, 2, 1)),
    (frame(849), (256, 2, 1, 2, 1)),
    (frame(850), (256, 4, 1, 2, 1)),
    (frame(1599), (256, 4, 1, 2, 1)),
    (frame(1600), (256, 8, 1, 2, 1)),
    (frame(4096), (256, 8, 1, 2, 1)),
    (frame(4097), (256, 8, 1, 0, 0)),
    (frame(8192), (256, 8, 1, 0, 0)),
    # default switches, equirectangular: the same workgroup thresholds
    (frame(499, model=1), (256, 1, 1, 2, 1)),
    (frame(1600, model=1), (256, 8, 1, 2, 1)),
    # one workgroup: registers and batched retries to 512 observations, 512 threads from 768 (perspective) / 1500 (equirectangular)
    (frame(512, groups=1), (256, 1, 1, 2, 1)),
    (frame(513, groups=1), (256, 1, 0, 0, 0)),
    (frame(767, groups=1), (256, 1, 0, 0, 0)),
    (frame(768, groups=1), (512, 1, 0, 0, 0)),
    (frame(1499, model=1, groups=1), (256, 1, 0, 0, 0)),
    (frame(1500, model=1, groups=1), (512, 1, 0, 0, 0)),
    (frame(768, model=1, groups=1), (256, 1, 0, 0, 0)),
    # forced workgroup counts around 2 * g * 256
    (frame(1024, groups=2), (256, 2, 1, 2, 1)),
    (frame(1025, groups=2), (256, 2, 1, 0, 0)),
    (frame(2048, groups=4), (256, 4, 1, 2, 1)),
    (frame(2049, groups=4), (256, 4, 1, 0, 0)),
    (frame(4096, groups=8), (256, 8, 1, 2, 1)),
    (frame(4097, groups=8), (256, 8, 1, 0, 0)),
    (frame(4096, groups=9), (256, 8, 1, 2, 1)),      # clamped to 8
    (frame(300, groups=9), (256, 8, 1, 2, 1)),
    # forced workgroup sizes
    (frame(2000, threads=512), (512, 8, 1, 0, 0)),   # eight workgroups of 512 threads (the 512-thread kernel ignores batch_retries)
    (frame(300, threads=512), (512, 1, 1, 0, 0)),
    (frame(1000, threads=256, groups=1), (256, 1, 0, 0, 0)),   # above the 512-thread threshold a forced 256 re-reads its records
    (frame(300, threads=256), (256, 1, 1, 2, 1)),
    (frame(300, threads=300), (256, 1, 1, 2, 1)),    # neither 256 nor 512: by size
    # the data-path and retry switches
    (frame(300, obs_regs=0), (256, 1, 1, 0, 0)),
    (frame(300, zero_copy=0), (256, 1, 1, 2, 0)),
    (frame(300, retries=0), (256, 1, 0, 2, 1)),
    (frame(2000, retries=0), (256, 8, 0, 2, 1)),
    (frame(2000, groups=1, retries=1), (512, 1, 1, 0, 0)),
    # the fallback attempt: one workgroup whatever the switches say, inputs through device memory
    (frame(2000, first=0), (512, 1, 0, 0, 0)),
    (frame(300, groups=8, first=0), (256, 1, 1, 2, 0)),
    (frame(1000, model=1, first=0), (256, 1, 0, 0, 0)),
    # the batch entries: one 256-thread workgroup per frame, records from memory, retries one by one
    (batch(), (256, 1, 0, 0, 0)),
    (batch(threads=512), (512, 1, 0, 0, 0)),
    (batch(groups=8), (256, 1, 0, 0, 0)),
    (batch(retries=1), (256, 1, 1, 0, 0)),
    (batch(retries=0, obs_regs=0, zero_copy=0), (256, 1, 0, 0, 0)),
]

# n -> (off_off, off_obs, in_bytes, off_out, off_nv, off_fl, out_bytes, off_part, total): 64-byte records from 128, the outputs on the next
# 256-byte boundary (pose, count at + 96, flags at + 128), the 2 * 8 * 56 exchange words on the next one
BLOCKS = [
    (0, (96, 128, 192, 256, 352, 384, 129, 512, 7680)),
    (1, (96, 128, 192, 256, 352, 384, 129, 512, 7680)),
    (300, (96, 128, 19328, 19456, 19552, 19584, 428, 19968, 27136)),
    (8192, (96, 128, 524416, 524544, 524640, 524672, 8320, 532992, 540160)),
]


@pytest.fixture(scope="module")
def answers():
    subprocess.check_call(["make", "-s", "-C", CPP, "pose_plan_host"])
    rows = [r for r, _ in LAUNCHES] + ["block:%d" % n for n, _ in BLOCKS]
    r = subprocess.run([os.path.join(CPP, "pose_plan_host")] + rows, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    return {row: tuple(int(v) for v in line.split()) for row, line in zip(rows, lines)}


@pytest.mark.parametrize("row,want", LAUNCHES, ids=[r for r, _ in LAUNCHES])
def test_launch_plan(answers, row, want):
    assert answers[row] == want


@pytest.mark.parametrize("n,want", BLOCKS, ids=["n%d" % n for n, _ in BLOCKS])
def test_block_layout(answers, n, want):
    got = answers["block:%d" % n]
    assert got == want
    off_off, off_obs, in_bytes, off_out, off_nv, off_fl, out_bytes, off_part, total = got
    assert off_obs % 64 == 0 and off_out % 256 == 0 and off_part % 256 == 0
    assert 96 <= off_off and off_off + 8 <= off_obs and off_obs + 64 * n <= in_bytes <= off_out      # pose, two offsets, the records
    assert off_out + 96 <= off_nv and off_nv + 4 <= off_fl and off_fl + n <= off_out + out_bytes <= off_part
    assert total == off_part + 8 * 2 * 8 * 56


def test_the_program_refuses_a_malformed_row(answers):
    exe = os.path.join(CPP, "pose_plan_host")
    for row in ("frame:0:300", "block:", "plan:1"):
        assert subprocess.run([exe, row], capture_output=True, timeout=60).returncode == 2
