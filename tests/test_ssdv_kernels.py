"""The SSDV kernels' resources, from the compiler's own metadata -- no GPU needed.

k_ssdv_scan and k_ssdv_append cross-compile for gfx950, spill no register of either kind and use no scratch, and k_ssdv_scan's registers and LDS let at
least four waves per SIMD stay resident; the test prints the figures of the build it runs on (NOTES.md has those of the build it was written with).
Metadata only: no instruction text is searched."""
import re

from test_kernel_resources import CSRC, kernel_table


def test_ssdv_kernels_have_no_scratch_no_spills_and_four_waves_per_simd(tmp_path):
    t = kernel_table(CSRC / "kernels" / "ssdv.hip", tmp_path)
    assert set(t) == {"k_ssdv_scan", "k_ssdv_append"}, sorted(t)
    txt = (tmp_path / "ssdv.s").read_text()
    meta = txt[txt.index("amdhsa.kernels:"):]
    blocks = re.split(r"\n  - \.agpr_count", meta)[1:]
    assert len(blocks) == 2
    for blk in blocks:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        k = next(v for n, v in t.items() if "%d%sE" % (len(n), n) in name)                  # (the mangled name holds the length-prefixed one)
        sgpr = int(re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
        sgpr_spill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        print(name, k, "sgpr", sgpr, "sgpr_spill", sgpr_spill, "lds", lds)
        assert k["spill"] == 0 and k["scratch"] == 0 and sgpr_spill == 0, (name, k, sgpr_spill)
        # four waves per SIMD: 512 registers a lane / 4 = 128; a workgroup is four waves (one per SIMD), so four workgroups per CU, 160 KB / 4 of LDS
        assert k["vgpr"] <= 128 and sgpr <= 102 and lds <= 160 * 1024 // 4, (name, k, sgpr, lds)
