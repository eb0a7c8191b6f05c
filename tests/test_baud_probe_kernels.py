"""The probe kernel's claims, from the compiler's own metadata -- no GPU needed.

k_baud_probe cross-compiles for gfx950, spills no register of either kind, uses no scratch, no atomics and -- behind the one comparison that makes a sign
bit -- no floating point; its cosine table and the history words lie in LDS."""
import re

from test_kernel_resources import CSRC, kernel_table


def test_baud_probe_kernel_has_no_scratch_and_no_spills(tmp_path):
    t = kernel_table(CSRC / "kernels" / "baud_probe.hip", tmp_path)
    assert set(t) == {"k_baud_probe"}, sorted(t)
    k = t["k_baud_probe"]
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] <= 128, k                       # 1024 threads per workgroup: four waves per SIMD
    txt = (tmp_path / "baud_probe.s").read_text()
    assert k["sgpr_spill"] == 0
    assert k["lds"] >= 4096                                                                         # the cosine table
    code = txt[:txt.index("amdhsa.kernels:")]
    assert "scratch_" not in code and "global_atomic" not in code and "flat_atomic" not in code and "ds_add" not in code
    assert "v_cmp_lt_f32" in code or "v_cmp_gt_f32" in code                                         # d > 0.0f
    floats = set(re.findall(r"\b(v_(?:add|sub|mul|fma|mac|fmac|pk_add|pk_mul|pk_fma|cvt)_[a-z0-9_]*f(?:16|32|64)[a-z0-9_]*)", code))
    assert not floats, floats
    assert "ds_read" in code or "ds_load" in code
