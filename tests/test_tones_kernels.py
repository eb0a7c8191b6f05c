"""The tone-filter demodulator kernel's resources, from the compiler's own metadata -- no GPU needed.

k_tones cross-compiles for gfx950, spills no register of either kind and uses no scratch; the test prints the figures of the build it runs on (NOTES.md
has those of the build it was written with)."""
from test_kernel_resources import CSRC, kernel_table


def test_tones_kernel_has_no_scratch_and_no_spills(tmp_path):
    t = kernel_table(CSRC / "kernels" / "tones.hip", tmp_path)
    assert set(t) == {"k_tones"}, sorted(t)
    k = t["k_tones"]
    sgpr, sgpr_spill, lds = k["sgpr"], k["sgpr_spill"], k["lds"]
    print("k_tones", k, "sgpr", sgpr, "sgpr_spill", sgpr_spill, "lds", lds)
    assert k["spill"] == 0 and k["scratch"] == 0 and sgpr_spill == 0, (k, sgpr_spill)
    assert k["vgpr"] <= 128 and sgpr <= 102, (k, sgpr)       # a workgroup of four waves per stream: four workgroups per CU have 128 registers a lane
    assert lds == 0                                           # no static LDS: the chunk's running sums are dynamic LDS, sized by the host
