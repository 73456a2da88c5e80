"""The resources of the pose-graph optimiser's kernels that DESIGN.md 3.19 quotes, read from the gfx950 code object hipcc emits here (no
device): no scratch, the register counts, and the LDS of the two slots rule 6's sums are broadcast through."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_posegraph_kernels_have_no_scratch_and_the_figures_design_quotes():
    import kernel_resources as kr
    rows = {("optimize" if "k_posegraph_optimize" in r[1] else "correct"): r for r in kr.collect(files={"pose_graph.hip"}) if "k_posegraph_" in r[1]}
    assert sorted(rows) == ["correct", "optimize"]
    for name, r in rows.items():
        print(name, "vgpr", r[2], "agpr", r[3], "sgpr", r[4], "scratch", r[5], "lds", r[6], "max workgroup", r[7])
    _, _, vgpr, agpr, sgpr, scratch, lds, max_wg = rows["optimize"]
    assert scratch == 0 and max_wg == 256
    # DESIGN.md 3.19 quotes these figures. One workgroup of four wavefronts runs the kernel, one per SIMD, so any count up to 512 registers costs
    # no occupancy that is wanted: the quoted figures themselves are held, and a change of the source or of the compiler that moves them has
    # to move DESIGN with them.
    assert (vgpr, agpr, sgpr) == (316, 60, 106)
    assert lds == 2 * 8                                   # the two broadcast slots
    _, _, vgpr, agpr, sgpr, scratch, lds, max_wg = rows["correct"]
    assert (vgpr, agpr, sgpr, scratch, lds, max_wg) == (62, 0, 15, 0, 0, 256)
