"""The unpack kernel's register claims, from the compiler's own metadata -- no GPU needed.

k_iq_unpack is a streaming kernel whose only way to hide memory latency is the number of waves: it must keep every wave slot (at most 64 registers),
spill nothing, and use neither scratch nor atomics."""
from test_kernel_resources import CSRC, kernel_table


def test_iq_unpack_kernel_keeps_every_wave_slot(tmp_path):
    t = kernel_table(CSRC / "kernels" / "iq_unpack.hip", tmp_path)
    assert set(t) == {"k_iq_unpack"}, sorted(t)
    k = t["k_iq_unpack"]
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] <= 64, k
    txt = (tmp_path / "iq_unpack.s").read_text()
    assert "scratch_" not in txt and "global_atomic" not in txt and "flat_atomic" not in txt
    assert "global_load_dwordx4" in txt and "global_store_dwordx4" in txt          # the vectors go as 16-byte loads and stores
