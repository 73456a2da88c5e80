"""The conjugate-gradient solver of the reduced camera system, the part that needs no device: the sequential reference
(tests/ba_pcg_ref.py) against a dense solve, openvslam_amd/csrc/ba_pcg_math.inc through a plain host compiler against the reference's
bits, and the host plan (ba_pcg_plan.inc) with the solver's edges under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import numpy as np
import pytest

import ba_pcg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvslam_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "ba_pcg_host.cc")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ba_pcg_host") / "ba_pcg_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ba_pcg_host_san") / "ba_pcg_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe, SRC])
    return exe


def _residual(S, g, x):
    return float(np.linalg.norm(S @ x - g) / np.linalg.norm(g))


@pytest.mark.parametrize("n,cond,max_iter", [(66, 1e2, 0), (390, 1e4, 0), (1026, 1e3, 0), (66, 1e6, 40 * 66)])
def test_reference_against_a_dense_solve_on_random_spectra(n, cond, max_iter):
    """R1: relative residual <= 100 tol = 1e-8 (ten times the worst value of the CPU experiment that chose tol). Found: 66 / 1e2: 6.2e-11
    in 69 iterations; 390 / 1e4: 8.4e-11 in 668; 1026 / 1e3: 8.8e-11 in 297; 66 / 1e6: 3.9e-11 in 518. The last one is given a cap of 40 n:
    block-Jacobi does nothing for a random basis, the count goes with sqrt(cond), and the default cap of 2 n = 132, which is sized for camera
    systems, stops it at a residual of 3.6e-5 (the test below holds that the cap is then reported). The solution agrees with
    numpy.linalg.solve within cond x residual (found: 8e-10, 2e-8, 3e-9, 4.5e-8)."""
    S, g = ref.case(n, cond)
    x, (iters, capped, ratio) = ref.solved(n, cond, max_iter)
    res = _residual(S, g, x)
    print("n %d cond %g: %d iterations, capped %s, residual %.3g, dn / d0 %.3g" % (n, cond, iters, capped, res, ratio))
    assert not capped
    assert res <= 100 * ref.TOL
    want = np.linalg.solve(S, g)
    assert np.abs(x - want).max() / np.abs(want).max() <= cond * res


@pytest.mark.parametrize("n", ref.BLOCK_SIZES)
def test_reference_on_block_dominant_systems(n):
    """R1 at the sizes of more than two workgroups of the lane-per-block kernels (3078: 513 blocks; 6144: the capacity): not capped, at least
    8 iterations (so that check_every = 7 spans two chunks), relative residual <= 100 tol. Found: 15 iterations at both sizes, residuals
    2.4e-11 and 7.1e-11. At 3078 the solution also agrees with numpy.linalg.solve within cond x residual (found: cond 38.5, 3.8e-10
    against 9.4e-10); no dense solve at 6144."""
    S, g = ref.block_case(n)
    x, (iters, capped, ratio) = ref.block_solved(n)
    res = _residual(S, g, x)
    print("block n %d: %d iterations, capped %s, residual %.3g, dn / d0 %.3g" % (n, iters, capped, res, ratio))
    assert not capped and 8 <= iters < 12 * (n // 6)
    assert res <= 100 * ref.TOL
    if n == 3078:
        want = np.linalg.solve(S, g)
        cond = float(np.linalg.cond(S))
        err = np.abs(x - want).max() / np.abs(want).max()
        print("cond %.3g, against the dense solve %.3g, bound %.3g" % (cond, err, cond * res))
        assert err <= cond * res


def test_reference_reports_the_cap_on_a_system_it_is_too_small_for():
    x, (iters, capped, ratio) = ref.solved(66, 1e6)
    assert iters == 132 and capped and ratio > ref.TOL ** 2


def test_reference_on_reduced_camera_systems(oracle):
    """R1: every system the 24-keyframe ring's ten LM trials solve (138 unknowns, cond 6.6e4): residual <= 1e-8 and fewer iterations than
    the cap. Found: 50 to 96 iterations against a cap of 276, worst residual 2.3e-10."""
    import global_ba_ref
    _, res = global_ba_ref.reference("ring24")
    assert len(res["systems"]) == 10
    worst, most = 0.0, 0
    for A, g in res["systems"]:
        x, (iters, capped, _) = ref.solve(A, g)
        worst, most = max(worst, _residual(A, g, x)), max(most, iters)
        assert not capped and iters < 12 * (len(g) // 6)
    print("worst residual %.3g, most iterations %d of %d" % (worst, most, 12 * (len(g) // 6)))
    assert worst <= 100 * ref.TOL


def test_reference_edges():
    rng = np.random.default_rng(3)
    S = ref.spd(rng, 12, 10.0)
    x, info = ref.solve(S, np.zeros(12))
    assert info == (0, False, 0.0) and not x.any()
    bad = S.copy()
    bad[7, 7] = -1.0
    with pytest.raises(ref.Failed):
        ref.solve(bad, np.ones(12))
    ind = np.eye(12)
    ind[np.arange(6), np.arange(6) + 6] = ind[np.arange(6) + 6, np.arange(6)] = -3.0
    with pytest.raises(ref.Failed):
        ref.solve(ind, np.ones(12))
    x, info = ref.solved(66, max_iter=3)
    assert info[0] == 3 and info[1] is True


def nonfinite_rhs(n):
    """case(n)'s right-hand side with a NaN, and with an Inf, in the first entry of the last block (1542: entry 1536)."""
    S, g = ref.case(n)
    out = []
    for v in (np.nan, np.inf):
        h = np.array(g)
        h[n - 6] = v
        out.append((S, h))
    return out


@pytest.mark.parametrize("n", [12, 1542])
def test_reference_edges_in_the_last_block(n):
    """P5 with the offending entry in the last block: every failure case raises; a right-hand side that is not finite is no failure but the
    outcome of g = 0 (P4's test is false at k = 0)."""
    for name, (S, g) in ref.failure_cases(n).items():
        with pytest.raises(ref.Failed):
            ref.solve(S, g)
    for S, g in nonfinite_rhs(n):
        x, info = ref.solve(S, g)
        assert info == (0, False, 0.0) and not x.any()


def _run_host(exe, tmp_path, cases):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:   # the arrays go out as they are: a Python list of a 3078-square matrix's entries would take seconds to build
        np.array([len(cases)], np.float64).tofile(f)
        for S, g, max_iter in cases:
            assert np.shape(S) == (len(g), len(g))
            np.array([len(g), ref.TOL, max_iter], np.float64).tofile(f)
            np.ascontiguousarray(S, np.float64).tofile(f)
            np.ascontiguousarray(g, np.float64).tofile(f)
    subprocess.check_call([exe, "solve", fin, fout])
    out, at, res = np.fromfile(fout), 0, []
    for S, g, _ in cases:
        n = len(g)
        res.append((out[at] == 1.0, out[at + 1:at + 1 + n], out[at + 1 + n:at + 4 + n]))
        at += 4 + n
    assert at == len(out)
    return res


def test_host_program_gives_the_references_bits(host, tmp_path):
    """R2: whole solves at every size the device test uses, and the three-iteration cap."""
    cases = [ref.case(n) + (0,) for n in ref.SIZES] + [ref.case(66) + (3,)]
    want = [ref.solved(n) for n in ref.SIZES] + [ref.solved(66, max_iter=3)]
    for (ok, x, info), (wx, (iters, capped, ratio)) in zip(_run_host(host, tmp_path, cases), want):
        assert ok
        assert np.array_equal(ref.bits(x), ref.bits(wx))
        assert info[0] == iters and bool(info[1]) == capped and ref.bits(info[2]) == ref.bits(ratio)


def test_host_program_gives_the_references_bits_at_513_blocks(host, tmp_path):
    """R2 on the block-dominant system of 3078 unknowns (the capacity is left to the device test: the host program has no workgroups)."""
    (ok, x, info), = _run_host(host, tmp_path, [ref.block_case(3078) + (0,)])
    wx, (iters, capped, ratio) = ref.block_solved(3078)
    assert ok
    assert np.array_equal(ref.bits(x), ref.bits(wx))
    assert info[0] == iters and bool(info[1]) == capped and ref.bits(info[2]) == ref.bits(ratio)


def test_host_program_edges_in_the_last_block(host, tmp_path):
    """The shared arithmetic decides the 1542-unknown failure cases and the right-hand sides that are not finite as the reference does."""
    fails = list(ref.failure_cases(1542).values())
    res = _run_host(host, tmp_path, [c + (0,) for c in fails + nonfinite_rhs(1542)])
    assert [ok for ok, _, _ in res] == [False] * len(fails) + [True, True]
    for ok, x, info in res[len(fails):]:
        assert not x.any() and info.tolist() == [0.0, 0.0, 0.0]


def test_host_plan_and_edges_under_the_sanitizers(host_san, tmp_path):
    """R3: the plan at 1, 170, 171 free keyframes, at the capacity and one beyond (nothing is allocated), bad arguments; then the solver's
    edges -- an indefinite matrix, a zero right-hand side, a non-positive diagonal block, a NaN, the cap -- and one solve's bits."""
    def plan(nf, tol="1e-10", max_iter=0, check_every=0):
        out = subprocess.check_output([host_san, "plan", str(nf), tol, str(max_iter), str(check_every)]).decode().split()
        return [int(v) for v in out]
    # status n n_blocks max_iter check_every grid_product grid_update arena_bytes ordered passes chunks
    assert plan(1) == [0, 6, 1, 12, 16, 1, 1, 12 * 256, 1, 13, 1]
    assert plan(170)[:7] == [0, 1020, 170, 2040, 16, 170, 1] and plan(170)[8:] == [1, 2041, 128]
    assert plan(171)[:7] == [0, 1026, 171, 2052, 16, 171, 1]
    cap = plan(1024)
    assert cap[:7] == [0, 6144, 1024, 12288, 16, 1024, 4] and cap[8] == 1
    # 36 + 6 x 6 doubles per block, two arrays of one double per block, the scalars and the words
    assert cap[7] == 1024 * 36 * 8 + 6 * 6144 * 8 + 2 * 1024 * 8 + 256 + 256
    assert plan(1025) == [-4]                     # OVS_ERR_CAPACITY
    assert plan(0) == [-1] and plan(-3) == [-1]   # OVS_ERR_INVALID
    assert plan(4, max_iter=3, check_every=7) == [0, 24, 4, 3, 7, 4, 1, 15 * 256, 1, 4, 1]
    assert plan(4, max_iter=20, check_every=7)[9:] == [21, 3]
    assert plan(4, max_iter=-1) == [-1] and plan(4, check_every=-1) == [-1]
    assert plan(4, tol="0") == [-1] and plan(4, tol="1") == [-1] and plan(4, tol="nan") == [-1]
    out = subprocess.check_output([host_san, "edges"]).decode().split("\n")
    assert out[:5] == ["indefinite 0", "zero_rhs 1 0 0 0 1", "bad_block 0", "nan 0", "cap 1 3 1"]
    (ok, x, info), = _run_host(host_san, tmp_path, [ref.case(66) + (0,)])
    assert ok and np.array_equal(ref.bits(x), ref.bits(ref.solved(66)[0]))
