"""The diversity combiner's kernels' resources, from the compiler's own metadata -- no GPU needed.

k_combine, k_combine_lags and k_combine_lags_reduce cross-compile for gfx950, spill no register of either kind and use no scratch; the test prints the
figures of the build it runs on (NOTES.md has those of the build it was written with)."""
from test_kernel_resources import CSRC, kernel_table


def test_combine_kernels_have_no_scratch_and_no_spills(tmp_path):
    t = kernel_table(CSRC / "kernels" / "combine.hip", tmp_path)
    assert set(t) == {"k_combine", "k_combine_lags", "k_combine_lags_reduce"}, sorted(t)
    for name, k in t.items():
        sgpr, sgpr_spill, lds = k["sgpr"], k["sgpr_spill"], k["lds"]
        print(name, k, "sgpr", sgpr, "sgpr_spill", sgpr_spill, "lds", lds)
        assert k["spill"] == 0 and k["scratch"] == 0 and sgpr_spill == 0, (name, k, sgpr_spill)
        assert k["vgpr"] <= 128 and sgpr <= 102, (name, k, sgpr)      # workgroups of four waves: four of them per CU have 128 registers a lane
        # static LDS only: the sign words of the longest window (256) and of the span a block of 256 lags needs (261); k_combine keeps nothing there
        assert lds <= 8 * (256 + 261) + 64 and (lds == 0) == (name == "k_combine"), (name, lds)
