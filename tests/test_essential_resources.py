"""The resources DESIGN.md 3.16 quotes for the two kernels of csrc/essential_solve.hip, read from the gfx950 code object hipcc emits here (no
device): no scratch, no AGPRs, one wavefront per workgroup, the 9 x 9 problem with its vectors in LDS, the registers."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# DESIGN.md 3.16
QUOTED = {"k_essential_hypotheses": dict(vgpr=120, sgpr=44, lds=1328), "k_essential_finish": dict(vgpr=144, sgpr=56, lds=1296)}


@pytest.fixture(scope="module")
def kernels():
    import kernel_resources as kr
    rows = kr.collect(files={"essential_solve.hip"})
    short = lambda name: re.search(r"k_essential_[a-z]+", name).group(0)   # (mangled where the toolchain has no demangler)
    return {short(name): dict(vgpr=v, agpr=a, sgpr=s, scratch=p, lds=g, max_wg=w) for (_, name, v, a, s, p, g, w) in rows}


def test_the_unit_has_exactly_its_two_kernels(kernels):
    assert sorted(kernels) == sorted(QUOTED)


@pytest.mark.parametrize("name", sorted(QUOTED))
def test_no_scratch_one_wavefront_and_the_quoted_figures(kernels, name):
    k = kernels[name]
    assert k["scratch"] == 0 and k["agpr"] == 0 and k["max_wg"] == 64
    assert {key: k[key] for key in QUOTED[name]} == QUOTED[name]


def test_the_hypothesis_kernel_keeps_four_waves_per_simd(kernels):
    assert kernels["k_essential_hypotheses"]["vgpr"] <= 128
