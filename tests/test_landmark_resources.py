"""The resources of the landmark upkeep's kernels that DESIGN.md 3.14 quotes, read from the metadata of the gfx950 code object hipcc emits here
(no device): no scratch, the register counts, the LDS of the camera-centre table and of a group's descriptors, and the workgroup sizes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_landmark_kernels_have_no_scratch_and_the_figures_design_quotes():
    import kernel_resources as kr
    rows = {}
    for _, name, vgpr, agpr, sgpr, scratch, lds, max_wg in kr.collect(files={"landmark_update.hip"}):
        key = next(k for k in ("k_landmark_geometry", "k_landmark_gather", "k_landmark_descriptorILi8E", "k_landmark_descriptorILi64E") if k in name)
        assert key not in rows
        rows[key] = (vgpr, agpr, sgpr, scratch, lds, max_wg)
        print(key, "vgpr", vgpr, "agpr", agpr, "sgpr", sgpr, "scratch", scratch, "lds", lds, "workgroup", max_wg)
    assert len(rows) == 4
    assert all(r[3] == 0 and r[1] == 0 for r in rows.values())   # no scratch, no accumulation registers
    # DESIGN.md 3.14 quotes these figures. A change of the source or of the compiler that moves them has to move DESIGN with them.
    assert rows["k_landmark_geometry"] == (52, 0, 38, 0, 256 * 24, 256)             # the 256 camera centres a workgroup holds in LDS
    assert rows["k_landmark_descriptorILi8E"] == (58, 0, 44, 0, 8 * 72 * 4, 64)     # eight groups of eight descriptors, a pad of 8 words each
    assert rows["k_landmark_descriptorILi64E"] == (42, 0, 38, 0, 128 * 32, 64)      # the first 128 descriptors of the landmark
    assert rows["k_landmark_gather"] == (8, 0, 22, 0, 0, 256)
    assert all(r[0] <= 64 for r in rows.values())   # 512 / 64: eight wavefronts per SIMD, the occupancy limit, for every kernel
