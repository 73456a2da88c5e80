"""The resources DESIGN.md 3.15 quotes for the two kernels of csrc/two_view_reconstruct.hip, read from the gfx950 code object hipcc emits here (no
device): no scratch, one wavefront per workgroup, no LDS (the 3 x 3 decomposition lives in registers), the registers."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# DESIGN.md 3.15
QUOTED = {"k_reconstruct_hypotheses": dict(vgpr=98, lds=0), "k_reconstruct_finish": dict(vgpr=92, lds=0)}


@pytest.fixture(scope="module")
def kernels():
    import kernel_resources as kr
    rows = kr.collect(files={"two_view_reconstruct.hip"})
    short = lambda name: re.search(r"k_reconstruct_[a-z]+", name).group(0)   # (mangled where the toolchain has no demangler)
    return {short(name): dict(vgpr=v, agpr=a, sgpr=s, scratch=p, lds=g, max_wg=w) for (_, name, v, a, s, p, g, w) in rows}


def test_the_unit_has_exactly_its_two_kernels(kernels):
    assert sorted(kernels) == sorted(QUOTED)


@pytest.mark.parametrize("name", sorted(QUOTED))
def test_no_scratch_one_wavefront_and_the_quoted_figures(kernels, name):
    k = kernels[name]
    assert k["scratch"] == 0 and k["max_wg"] == 64
    assert k["agpr"] == 0 and k["vgpr"] == QUOTED[name]["vgpr"] and k["lds"] == QUOTED[name]["lds"]
    assert k["vgpr"] <= 128                        # four waves per SIMD or more
