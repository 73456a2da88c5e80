"""The resources of the triangulator's kernel that DESIGN.md 3.12 quotes, read from the metadata of the gfx950 code object hipcc emits here (no
device): no scratch, the register counts, and the LDS of a wavefront's problem records."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_triangulate_kernel_has_no_scratch_and_the_figures_design_quotes():
    import kernel_resources as kr
    rows = [r for r in kr.collect(files={"triangulate.hip"}) if "k_triangulate" in r[1]]
    assert len(rows) == 1
    _, _, vgpr, agpr, sgpr, scratch, lds, max_wg = rows[0]
    print("k_triangulate: vgpr", vgpr, "agpr", agpr, "sgpr", sgpr, "scratch", scratch, "lds", lds)
    assert scratch == 0 and max_wg == 64
    # DESIGN.md 3.12 quotes these figures: the 4 x 4 system and its vectors (32 doubles) with a match's inputs stay under 256 registers, so three
    # wavefronts fit a SIMD. A change of the source or of the compiler that moves them has to move DESIGN with them.
    assert vgpr <= 168 and agpr == 0          # 512 / 168 = 3 wavefronts per SIMD
    assert (vgpr, sgpr) == (146, 74)
    assert lds == 64 * 352 == 22528           # a record of 44 doubles for each of the at most 64 problems a wavefront's matches belong to
