"""The tone search kernel's resources, from the compiler's own metadata -- no GPU needed.

k_tone_search cross-compiles for gfx950, spills no register of either kind and uses no scratch; the test prints the figures of the build it runs on
(NOTES.md has those of the build it was written with)."""
from test_kernel_resources import CSRC, kernel_table


def test_tone_search_kernel_has_no_scratch_and_no_spills(tmp_path):
    t = kernel_table(CSRC / "kernels" / "tone_search.hip", tmp_path)
    assert set(t) == {"k_tone_search"}, sorted(t)
    k = t["k_tone_search"]
    sgpr, sgpr_spill, lds = k["sgpr"], k["sgpr_spill"], k["lds"]
    print("k_tone_search", k, "sgpr", sgpr, "sgpr_spill", sgpr_spill, "lds", lds)
    assert k["spill"] == 0 and k["scratch"] == 0 and sgpr_spill == 0, (k, sgpr_spill)
    assert k["vgpr"] <= 256, k                                # one wave per SIMD (waves_per_eu(1, 1)): 64 registers of samples and the twiddles in flight
    assert lds == 64 * 65 * 4                                 # the transpose plane of the wave's own, nothing else
    txt = (tmp_path / "tone_search.s").read_text()
    assert "flat_load" not in txt and "flat_store" not in txt  # every access is a global one: a flat one would make the LDS waits wait for memory too
