"""The LDS image of the low-pass kernel as host arithmetic (hd_host_fir_demod_lds_bytes / hd_host_fir_demod_max_taps, csrc/host/fir_lds.hpp), and the
compiler's own figures for k_fir_demod -- no GPU needed.

The engine derives the longest low-pass it runs (hd_engine_lowpass_taps_max) from these two functions and the device's LDS per workgroup, and
launch_fir_demod sizes its launch with the same formula: if the inverse were off by one tap, or the kernel's static LDS more than the formula assumes,
the longest admitted filter would ask for a launch the device cannot make.  Metadata only: no instruction text is searched."""
import pytest

from test_kernel_resources import CSRC, kernel_table


@pytest.fixture(scope="module")
def hd():
    from habdec_amd.build import build
    build()
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


def total(hd, taps):
    dyn, static = hd.fir_demod_lds_bytes(taps)
    return dyn + static


@pytest.mark.parametrize("limit", [64 * 1024, 160 * 1024])
def test_max_taps_is_the_largest_odd_count_that_fits(hd, limit):
    T = hd.fir_demod_max_taps(limit)
    assert T % 2 == 1 and 4097 < T <= 0xFFFF, T
    assert total(hd, T) <= limit < total(hd, T + 2), (T, total(hd, T), total(hd, T + 2))
    # ... and by search, without the inverse: the image grows by one complex sample per tap
    fits = [t for t in range(1, 0x10000, 2) if total(hd, t) <= limit]
    assert fits[-1] == T and fits == list(range(1, T + 1, 2))


def test_image_grows_by_one_complex_sample_per_tap_and_small_limits_admit_nothing(hd):
    dyn1, static = hd.fir_demod_lds_bytes(1)
    assert hd.fir_demod_lds_bytes(0) == (dyn1, static)                       # a launch in which no stream filters: the image of one tap
    assert all(hd.fir_demod_lds_bytes(t + 1)[0] - hd.fir_demod_lds_bytes(t)[0] == 8 for t in (1, 160, 4097, 18898, 65534))
    assert dyn1 > 1536 * 8                                                    # a tile of 1536 outputs' inputs at the least
    assert hd.fir_demod_max_taps(dyn1 + static - 1) == 0 and hd.fir_demod_max_taps(0) == 0
    assert hd.fir_demod_max_taps(dyn1 + static) == 1 and hd.fir_demod_max_taps(dyn1 + static + 8) == 1 and hd.fir_demod_max_taps(dyn1 + static + 16) == 3
    # the engine caps its limit at the sixteen bits StreamCall::fir_taps_prev keeps (a static assertion in fir_lds.hpp holds the 160 KB figure against them;
    # sc_pack_taps_prev itself has no host door): a device with far more LDS must not lift it -- the inverse alone goes on growing
    assert hd.fir_demod_max_taps(1 << 20) > 0xFFFF


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_fir_demod_static_lds_is_what_the_host_formula_assumes_and_nothing_spills(hd, tmp_path, fast):
    t = kernel_table(CSRC / "kernels" / "fir_demod.hip", tmp_path, fast)
    k = t["k_fir_demod"]
    print("k_fir_demod", "fast" if fast else "exact", k)
    assert k["lds"] == hd.fir_demod_lds_bytes(1)[1], k
    assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
    for name in ("k_lp_gather", "k_lp_taps_gather", "k_lp_mul", "k_fft_feed", "k_fetch_params"):
        assert t[name]["lds"] == 0 and t[name]["spill"] == 0 and t[name]["scratch"] == 0, (name, t[name])
