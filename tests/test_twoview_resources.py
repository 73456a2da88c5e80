"""The resources DESIGN.md 3.13 quotes for the two kernels of csrc/two_view_solve.hip, read from the gfx950 code object hipcc emits here (no
device): no scratch, one wavefront per workgroup, the registers and the LDS of the 9 x 9 eigenproblem."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# DESIGN.md 3.13; LDS: a 9 x 9 matrix and its vectors plus a hypothesis's eight indices; H's and F's refit side by side
QUOTED = {"k_twoview_hypotheses": dict(vgpr=128, lds=8 * (81 + 81) + 4 * 8), "k_twoview_finish": dict(vgpr=244, lds=2 * 8 * (81 + 81))}


@pytest.fixture(scope="module")
def kernels():
    import kernel_resources as kr
    rows = kr.collect(files={"two_view_solve.hip"})
    short = lambda name: re.search(r"k_twoview_[a-z]+", name).group(0)   # (mangled where the toolchain has no demangler)
    return {short(name): dict(vgpr=v, agpr=a, sgpr=s, scratch=p, lds=g, max_wg=w) for (_, name, v, a, s, p, g, w) in rows}


def test_the_unit_has_exactly_its_two_kernels(kernels):
    assert sorted(kernels) == sorted(QUOTED)


@pytest.mark.parametrize("name", sorted(QUOTED))
def test_no_scratch_one_wavefront_and_the_quoted_figures(kernels, name):
    k = kernels[name]
    assert k["scratch"] == 0 and k["max_wg"] == 64
    assert k["agpr"] == 0 and k["vgpr"] == QUOTED[name]["vgpr"] and k["lds"] == QUOTED[name]["lds"]
    assert k["vgpr"] <= 256                        # two waves per SIMD or more
