"""k_describe's residency is no longer set by its LDS: the row-blurred patch takes the patch's place, so a one-wave workgroup holds one
3 440-byte block and the CU's 32 wave slots are the limit. Read from the gfx950 code object hipcc emits here (no device), as
tests/test_kernel_resources.py reads the other budgets."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_k_describe_fits_32_waves_per_cu():
    import kernel_resources as kr
    rows = {name: dict(vgpr=v, agpr=a, scratch=p, lds=g) for (_, name, v, a, _s, p, g, _w) in kr.collect(files={"orb_describe.hip"})}
    desc = rows["ovs::k_describe"]
    assert desc["scratch"] == 0
    assert desc["vgpr"] <= 32                    # 512 / 32 = 16 waves per SIMD by registers: far from binding
    assert desc["lds"] <= 160 * 1024 // 32       # 5 120 B: thirty-two one-wave workgroups fit the CU's 160 KiB
