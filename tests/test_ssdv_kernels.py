"""The SSDV kernels' resources, from the compiler's own metadata -- no GPU needed.

k_ssdv_scan and k_ssdv_append cross-compile for gfx950, spill no register of either kind and use no scratch, and k_ssdv_scan's registers and LDS let at
least four waves per SIMD stay resident; the test prints the figures of the build it runs on (NOTES.md has those of the build it was written with).
Metadata only: no instruction text is searched."""
from test_kernel_resources import CSRC, kernel_table


def test_ssdv_kernels_have_no_scratch_no_spills_and_four_waves_per_simd(tmp_path):
    t = kernel_table(CSRC / "kernels" / "ssdv.hip", tmp_path)
    assert set(t) == {"k_ssdv_scan", "k_ssdv_append"}, sorted(t)
    for name, k in t.items():
        sgpr, sgpr_spill, lds = k["sgpr"], k["sgpr_spill"], k["lds"]
        print(name, k, "sgpr", sgpr, "sgpr_spill", sgpr_spill, "lds", lds)
        assert k["spill"] == 0 and k["scratch"] == 0 and sgpr_spill == 0, (name, k, sgpr_spill)
        # four waves per SIMD: 512 registers a lane / 4 = 128; a workgroup is four waves (one per SIMD), so four workgroups per CU, 160 KB / 4 of LDS
        assert k["vgpr"] <= 128 and sgpr <= 102 and lds <= 160 * 1024 // 4, (name, k, sgpr, lds)
