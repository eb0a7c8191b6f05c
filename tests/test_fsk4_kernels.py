"""The 4FSK modem's kernels' resources, from the compiler's own metadata -- no GPU needed.

k_fsk4_slots and k_fsk4_frames cross-compile for gfx950, spill no register of either kind and use no scratch; the test prints the figures of the build
it runs on (NOTES.md has those of the build it was written with)."""
from test_kernel_resources import CSRC, kernel_table


def test_fsk4_kernels_have_no_scratch_and_no_spills(tmp_path):
    t = kernel_table(CSRC / "kernels" / "fsk4.hip", tmp_path)
    assert set(t) == {"k_fsk4_slots", "k_fsk4_frames"}, sorted(t)
    for name, k in sorted(t.items()):
        print(name, k)
        assert k["spill"] == 0 and k["scratch"] == 0 and k["sgpr_spill"] == 0, (name, k)
        assert k["vgpr"] <= 128 and k["sgpr"] <= 102, (name, k)      # workgroups of four waves: four per CU have 128 registers a lane
    assert t["k_fsk4_slots"]["lds"] == 0                              # no static LDS: the chunk's running sums are dynamic LDS, sized by the host
    # four candidates' soft bits, gathered words and per-word results: eight workgroups of the frame kernel fit a CU's 160 KB
    assert 0 < t["k_fsk4_frames"]["lds"] <= 20 * 1024, t["k_fsk4_frames"]
