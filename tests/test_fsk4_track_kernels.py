"""The tone tracker's kernel's resources, from the compiler's own metadata -- no GPU needed.

k_fsk4_comb cross-compiles for gfx950, spills no register of either kind and uses no scratch; the test prints the figures of the build it runs on
(NOTES.md has those of the build it was written with, and k_fsk4_slots' with its phase words)."""
from test_kernel_resources import CSRC, kernel_table


def test_comb_kernel_has_no_scratch_and_no_spills(tmp_path):
    t = kernel_table(CSRC / "kernels" / "fsk4_track.hip", tmp_path)
    assert set(t) == {"k_fsk4_comb"}, sorted(t)
    k = t["k_fsk4_comb"]
    print("k_fsk4_comb", k)
    assert k["spill"] == 0 and k["scratch"] == 0 and k["sgpr_spill"] == 0, k
    assert k["vgpr"] <= 128 and k["sgpr"] <= 102, k                  # a workgroup of four waves
    # q, its prefix sums and the window sums, 16 KiB each, and the reductions' words: three workgroups fit a CU's 160 KB
    assert 48 * 1024 <= k["lds"] <= 50 * 1024, k
    s = kernel_table(CSRC / "kernels" / "fsk4.hip", tmp_path)["k_fsk4_slots"]
    print("k_fsk4_slots", s)
