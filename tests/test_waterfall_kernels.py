"""The waterfall kernels' resource claims, from the compiler's own metadata -- no GPU needed.

k_waterfall_detect runs one workgroup of 256 threads per row: four waves, one per SIMD of a CU.  Two workgroups resident per CU are two waves per SIMD,
so each wave may hold at most 512 / 2 = 256 vector registers; the 16 keys a lane keeps and the select's few counters need far fewer, and the stated
design bound of 64 keeps every one of a SIMD's eight wave slots open (LDS, 21 KiB per workgroup, then allows seven workgroups per CU)."""
import re

from test_kernel_resources import CSRC, kernel_table

WORKGROUP = 256                                  # kWfThreads
WAVES_PER_SIMD_PER_WORKGROUP = WORKGROUP // 64 // 4
TWO_WORKGROUPS_VGPR = 512 // (2 * WAVES_PER_SIMD_PER_WORKGROUP)


def test_waterfall_kernels(tmp_path):
    src = CSRC / "kernels" / "waterfall.hip"
    assert re.search(r"kWfThreads = (\d+)", src.read_text()).group(1) == str(WORKGROUP)
    t = kernel_table(src, tmp_path)
    assert set(t) == {"k_waterfall_detect", "k_waterfall_hits"}, sorted(t)
    for k in t:
        assert t[k]["spill"] == 0 and t[k]["scratch"] == 0, (k, t[k])
    assert TWO_WORKGROUPS_VGPR == 256 and t["k_waterfall_detect"]["vgpr"] <= TWO_WORKGROUPS_VGPR, t
    assert t["k_waterfall_detect"]["vgpr"] <= 64 and t["k_waterfall_hits"]["vgpr"] <= 64, t
    txt = (tmp_path / "waterfall.s").read_text()
    assert "scratch_" not in txt
    for atomic in ("global_atomic_add_f32", "global_atomic_pk_add", "_fmin", "_fmax", "atomic_add_f", "atomic_pk"):
        assert atomic not in txt, atomic
    atomics = [ln.split()[0] for ln in txt.splitlines() if re.match(r"\s+(global|flat|buffer)_atomic", ln)]
    assert atomics and set(atomics) <= {"global_atomic_add", "global_atomic_add_u32"}, atomics     # whole mnemonics: the hit counters' integer add, nothing else
    assert "ds_add_u32" in txt                                               # ... and they are there
    assert "v_fma_f32" not in txt and "v_pk_fma_f32" not in txt              # floor and level: each product and sum rounded once
    # LDS per workgroup: the row (16 KiB), four histograms (4 KiB), a few words -- two workgroups and more fit a CU's 160 KiB
    lds = t["k_waterfall_detect"]["lds"]
    assert 20 * 1024 <= lds <= 21 * 1024 and 2 * lds <= 160 * 1024, lds
