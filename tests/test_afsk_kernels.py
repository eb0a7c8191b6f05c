"""The AFSK / AX.25 modem's kernels' resources, from the compiler's own metadata -- no GPU needed.

k_afsk_slots, k_afsk_gate and k_afsk_frames cross-compile for gfx950, spill no register of either kind and use no scratch; the test prints the figures
of the build it runs on (NOTES.md has those of the build it was written with: 41 / 21 / 37 VGPRs, 59 / 35 / 58 SGPRs)."""
import ctypes as C

from test_kernel_resources import CSRC, kernel_table

# Registers a lane.  A SIMD's 512 VGPRs a lane hold eight waves at 64 and below: the frame kernel's waves hide one another's walks and ring reads, the
# slot kernel's two workgroups a CU (by LDS) are two waves a SIMD and nowhere near it.  The bounds are the next allocation steps above the build's
# figures that keep that occupancy, not the 128 a four-wave workgroup could have.
VGPR_BOUND = {"k_afsk_slots": 64, "k_afsk_gate": 32, "k_afsk_frames": 48}


def test_afsk_kernels_have_no_scratch_and_no_spills(tmp_path):
    t = kernel_table(CSRC / "kernels" / "afsk.hip", tmp_path)
    assert set(t) == set(VGPR_BOUND), sorted(t)
    for name, k in sorted(t.items()):
        print(name, k)
        assert k["spill"] == 0 and k["scratch"] == 0 and k["sgpr_spill"] == 0, (name, k)
        assert k["vgpr"] <= VGPR_BOUND[name] and k["sgpr"] <= 80, (name, k)
    assert t["k_afsk_slots"]["lds"] == 0                              # no static LDS: the chunk's running sums are dynamic LDS, sized by the host
    assert 0 < t["k_afsk_gate"]["lds"] <= 64                          # the four waves' counts
    # four candidates' packed levels (100 words), least confident lists (64) and frame bytes (83): 3952 bytes, forty workgroups to a CU's 160 KB --
    # the confidences stay in the slot ring
    assert 0 < t["k_afsk_frames"]["lds"] <= 4 * 1024, t["k_afsk_frames"]


def test_slot_kernel_dynamic_lds_lets_two_workgroups_share_a_cu():
    """What the launcher asks for: 16 (cap + 1 rounded up to 4) + 4096 + 64 bytes.  A whole chunk is 69760 bytes, two workgroups in a CU's 160 KB."""
    import habdec_amd
    f = habdec_amd.lib().hd_debug_afsk_slot_lds
    f.restype, f.argtypes = C.c_uint32, [C.c_uint32]
    assert f(4096) == 16 * 4100 + 4096 + 64 == 69760 and 2 * f(4096) <= 160 * 1024
    assert f(1) == 16 * 4 + 4096 + 64 and f(63) == 16 * 64 + 4160 and f(64) == 16 * 68 + 4160
    assert f(0) == 0 and f(4097) == 0                                 # no such launch
