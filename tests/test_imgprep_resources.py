"""The resources DESIGN.md 3.18 quotes for the kernels of csrc/image_prep.hip, read from the gfx950 code object hipcc emits here (no device):
exactly the six specialisations of k_image_prep by {rectify, channels}, no scratch, no AGPRs, no LDS, 256 threads, the registers."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# (rectify, channels) -> registers
QUOTED = {(1, 1): dict(vgpr=30, sgpr=32), (1, 3): dict(vgpr=46, sgpr=64), (1, 4): dict(vgpr=34, sgpr=66),
          (0, 1): dict(vgpr=11, sgpr=26), (0, 3): dict(vgpr=20, sgpr=30), (0, 4): dict(vgpr=20, sgpr=30)}


@pytest.fixture(scope="module")
def kernels():
    import kernel_resources as kr
    out = {}
    for (_, name, v, a, s, p, g, w) in kr.collect(files={"image_prep.hip"}):
        m = re.search(r"k_image_prep(?:ILb([01])ELi([134])E|<(true|false), ([134])>)", name)   # mangled where the toolchain has no demangler
        assert m, name
        key = (int(m.group(1)), int(m.group(2))) if m.group(1) is not None else (int(m.group(3) == "true"), int(m.group(4)))
        assert key not in out
        out[key] = dict(vgpr=v, agpr=a, sgpr=s, scratch=p, lds=g, max_wg=w)
    return out


def test_the_unit_has_exactly_its_six_specialisations(kernels):
    assert sorted(kernels) == sorted(QUOTED)


@pytest.mark.parametrize("key", sorted(QUOTED))
def test_no_scratch_no_agprs_no_lds_and_the_quoted_registers(kernels, key):
    k = kernels[key]
    assert k["scratch"] == 0 and k["agpr"] == 0 and k["lds"] == 0 and k["max_wg"] == 256
    assert {q: k[q] for q in QUOTED[key]} == QUOTED[key]


def test_every_specialisation_keeps_eight_waves_per_simd(kernels):
    assert max(k["vgpr"] for k in kernels.values()) <= 64
