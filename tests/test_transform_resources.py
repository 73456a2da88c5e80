"""The resources of the Sim3 transform optimiser's kernel that DESIGN.md 3.11 quotes, read from the gfx950 code object hipcc emits here (no
device): no scratch, the register counts, and the LDS of the 14 perturbed states and a lane's Jacobian entries."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_transform_kernel_has_no_scratch_and_the_figures_design_quotes():
    import kernel_resources as kr
    rows = [r for r in kr.collect(files={"sim3_opt.hip"}) if "k_sim3_optimize" in r[1]]
    assert len(rows) == 1
    _, _, vgpr, agpr, sgpr, scratch, lds, max_wg = rows[0]
    print("k_sim3_optimize: vgpr", vgpr, "agpr", agpr, "sgpr", sgpr, "scratch", scratch, "lds", lds)
    assert scratch == 0 and max_wg == 64
    # DESIGN.md 3.11 quotes these figures. The kernel is above 256 registers either way (one wavefront per SIMD, which is what a handful of
    # one-wave problems needs), so no occupancy tier gives a ceiling: the quoted figures themselves are held, and a change of the source or
    # of the compiler that moves them has to move DESIGN with them.
    assert (vgpr, agpr, sgpr) == (379, 123, 106)
    assert lds == 14 * 136 + 28 * 64 * 8 == 16240   # the 14 perturbed states (17 doubles each) and 28 Jacobian entries per lane
