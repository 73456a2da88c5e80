"""solve._pack, the one packer under the six batch calls of openvslam_amd.solve: offsets from the count key, every per-match array in one
contiguous (T, width) array of its dtype, the caller's ValueError when an array disagrees. Host only: no device, the library is not loaded."""
import numpy as np
import pytest

from openvslam_amd import solve

# what each of the six batch functions hands to _pack: its arrays, its count key, its error text
CALLERS = {
    "sim3": (solve._SIM3_ARRAYS, "thr1", "p1, p2, thr1 and thr2 of a problem must have one entry per match"),
    "pnp": (solve._PNP_ARRAYS, "max_cos_error", "bearings, pos_w and max_cos_error of a problem must have one entry per match"),
    "transform": (solve._OPT_ARRAYS, "w1", "p1, p2, obs1, obs2, w1 and w2 of a problem must have one entry per match"),
    "triangulate": (solve._TRI_ARRAYS, "x_right_1", "every per-match array of a problem must have one entry per match"),
    "two_view": (solve._TWO_VIEW_ARRAYS, "x1", "x1 and x2 of a problem must have one entry per match"),
    "essential": (solve._ESSENTIAL_ARRAYS, "b1", "b1 and b2 of a problem must have one entry per match"),
    "reconstruct": (solve._REC_ARRAYS, "inlier", "every per-match array of a problem must have one entry per match"),
}


def problem(arrays, n, base):
    """n matches of every array as nested lists (neither the dtype nor contiguous), entry (i, c) of array a being base + 100 a + 10 i + c."""
    return {key: [[base + 100 * a + 10 * i + c for c in range(w)] for i in range(n)] for a, (key, _, w) in enumerate(arrays)}


@pytest.mark.parametrize("name", sorted(CALLERS))
def test_offsets_dtypes_widths_and_order(name):
    arrays, count_key, error = CALLERS[name]
    problems = [problem(arrays, n, base) for n, base in ((0, 0), (1, 1), (3, 2))]
    P, offsets, T, packed = solve._pack(problems, arrays, count_key, error)
    assert (P, T) == (3, 4) and offsets.dtype == np.int32 and offsets.tolist() == [0, 0, 1, 4]
    assert len(packed) == len(arrays)
    for a, ((key, dt, w), got) in enumerate(zip(arrays, packed)):
        assert got.dtype == dt and got.shape == (4, w) and got.flags["C_CONTIGUOUS"], key
        want = [[base + 100 * a + 10 * i + c for c in range(w)] for n, base in ((1, 1), (3, 2)) for i in range(n)]
        assert got.tolist() == np.asarray(want, dt).tolist(), key


@pytest.mark.parametrize("name", sorted(CALLERS))
def test_no_match_at_all_gives_empty_arrays_of_the_width(name):
    arrays, count_key, error = CALLERS[name]
    for problems in ([], [problem(arrays, 0, 0)], [problem(arrays, 0, 0), problem(arrays, 0, 0)]):
        P, offsets, T, packed = solve._pack(problems, arrays, count_key, error)
        assert (P, T) == (len(problems), 0) and offsets.tolist() == [0] * (len(problems) + 1)
        assert [(a.shape, a.dtype) for a in packed] == [((0, w), np.dtype(dt)) for _, dt, w in arrays]


@pytest.mark.parametrize("name", sorted(CALLERS))
def test_a_mismatched_array_raises_the_callers_text(name):
    arrays, count_key, error = CALLERS[name]
    for key, _, w in arrays:
        if key == count_key:
            continue
        problems = [problem(arrays, 1, 0), problem(arrays, 3, 1)]
        problems[1][key] = problems[1][key][:2]   # one row short in the second problem
        with pytest.raises(ValueError) as e:
            solve._pack(problems, arrays, count_key, error)
        assert str(e.value) == error


def test_flat_input_of_the_right_size_is_taken_row_by_row():
    arrays, count_key, error = CALLERS["essential"]
    q = {"b1": np.arange(6, dtype=np.float32), "b2": np.arange(6, 12)[::-1]}   # flat, another dtype, a negative stride
    P, offsets, T, (b1, b2) = solve._pack([q], arrays, count_key, error)
    assert offsets.tolist() == [0, 2] and b1.tolist() == [[0, 1, 2], [3, 4, 5]] and b2.tolist() == [[11, 10, 9], [8, 7, 6]]
    assert b1.dtype == b2.dtype == np.float64 and b1.flags["C_CONTIGUOUS"] and b2.flags["C_CONTIGUOUS"]


def test_the_batch_functions_return_nothing_for_no_problem():
    # the P == 0 short-circuit comes before any handle: no device is touched
    assert solve.solve_sim3_batch([], False) == [] and solve.solve_pnp_batch([]) == [] and solve.optimize_transform_batch([], False) == []
    assert solve.triangulate_batch([], 1.8) == [] and solve.solve_two_view_batch([]) == [] and solve.solve_essential_batch([]) == []
    assert solve.reconstruct_two_view_batch([]) == []
