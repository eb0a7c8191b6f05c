"""The first stage with the rotation at the input rate in its staging loop (k_decimate_tuned, kernels/decimate.hip), from the compiler's own metadata:
all eight first-stage shapes compile for gfx950 in both arithmetic modes without spills or scratch, and the single-wave shapes keep the occupancy of the
untuned kernel they stand in for.  No GPU needed: hipcc cross-compiles a device-only listing, read the way tests/test_kernel_resources.py reads it."""
import pytest

from test_kernel_resources import CSRC, kernel_table

SHAPES = ["2,69,256", "4,139,256", "8,280,256", "8,54,256", "16,107,128", "32,212,64", "32,174,64", "64,348,64"]
CU_LDS = 160 * 1024


def lds_bytes(table: dict):
    """kernel name as kernel_table spells it -> static LDS of a workgroup"""
    return {name: k["lds"] for name, k in table.items()}


def workgroups_per_cu(vgpr: int, lds: int, lanes: int) -> int:
    """Resident workgroups of one kernel on a CU: 512 vector registers per lane and SIMD (allocated in blocks of 8), four SIMDs, 160 KB of LDS."""
    waves_per_simd = min(8, 512 // ((vgpr + 7) // 8 * 8))
    by_regs = waves_per_simd * 4 // (lanes // 64)
    return min(by_regs, CU_LDS // lds) if lds else by_regs


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_tuned_first_stages_do_not_spill_and_keep_their_occupancy(tmp_path, fast):
    t = kernel_table(CSRC / "kernels" / "decimate.hip", tmp_path, fast)
    listing = (tmp_path / "decimate.s").read_text()
    lds = lds_bytes(t)
    for shape in SHAPES:
        k, u = f"k_decimate_tuned<{shape}>", f"k_decimate<{shape}>"
        assert k in t, (k, sorted(x for x in t if x.startswith("k_decimate")))
        assert t[k]["spill"] == 0 and t[k]["scratch"] == 0 and t[k]["vgpr"] <= 256 + 256 * (shape == "64,348,64"), (k, t[k])
        assert t[u]["spill"] == 0 and t[u]["scratch"] == 0, (u, t[u])            # (the untuned instantiations are what they were)
        lanes = int(shape.split(",")[2])
        if lanes == 64:
            # /32: two waves per SIMD, eight workgroups per CU; /64 (its accumulators take more than 256 registers): one and four
            assert t[k]["vgpr"] <= (512 if shape == "64,348,64" else 256), (k, t[k])
            assert lds[k] == lds[u], (k, lds[k], lds[u])                          # the tables are not copied into these workgroups' LDS
            assert workgroups_per_cu(t[k]["vgpr"], lds[k], 64) == workgroups_per_cu(t[u]["vgpr"], lds[u], 64), (k, t[k], lds[k], t[u], lds[u])
        else:
            assert lds[k] == lds[u] + 4096, (k, lds[k], lds[u])                   # ... and into these they are: [C | F], 2 x 256 (cos, sin)
    if not fast:
        # exact mode: separately rounded multiply and add everywhere -- the rotation included
        assert listing.count("v_pk_fma_f32") == 0
    else:
        # fast mode fuses the FIR sums only: the rotation's products and sums stay separately rounded, so the tuned kernels carry the packed
        # multiplies and adds of tune.h beside the fused FIR (k_decimate<2,69,256> in fast mode has no v_pk_mul_f32 at all)
        body = listing[listing.index("k_decimate_tunedILi2ELi69ELi256"):]
        body = body[:body.index(".amdhsa_kernel")]
        assert body.count("v_pk_fma_f32") > 0 and body.count("v_pk_mul_f32") + body.count("v_mul_f32") >= 8, (body.count("v_pk_mul_f32"), body.count("v_mul_f32"))
