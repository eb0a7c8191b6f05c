"""The clocked decoder kernel's resources, from the compiler's own metadata -- no GPU needed.

k_clocked cross-compiles for gfx950, spills no register of either kind and uses no scratch.  The build this was written with (NOTES.md): 32 VGPRs,
73 SGPRs, no static LDS; the test prints the figures of the build it runs on."""
from test_kernel_resources import CSRC, kernel_table


def test_clocked_kernel_has_no_scratch_and_no_spills(tmp_path):
    t = kernel_table(CSRC / "kernels" / "clocked.hip", tmp_path)
    assert set(t) == {"k_clocked"}, sorted(t)
    k = t["k_clocked"]
    sgpr, sgpr_spill, lds = k["sgpr"], k["sgpr_spill"], k["lds"]
    print("k_clocked", k, "sgpr", sgpr, "sgpr_spill", sgpr_spill, "lds", lds)
    assert k["spill"] == 0 and k["scratch"] == 0 and sgpr_spill == 0, (k, sgpr_spill)
    assert k["vgpr"] <= 64 and sgpr <= 102, (k, sgpr)        # one wave per stream: eight waves per SIMD have 64 registers each
    assert lds == 0                                           # no static LDS: the launch's window of running sums is dynamic LDS, sized by the host
