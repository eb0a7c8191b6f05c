"""The survey kernels' register claims, from the compiler's own metadata -- no GPU needed.

k_survey keeps the 64-point register array AND 64 float accumulators per lane: it is built for one wave per SIMD (the whole 512-entry register file),
and must neither spill nor touch scratch there."""
from test_kernel_resources import CSRC, kernel_table


def test_survey_kernels_do_not_spill(tmp_path):
    t = kernel_table(CSRC / "kernels" / "survey.hip", tmp_path)
    assert set(t) == {"k_survey", "k_survey_reduce"}, sorted(t)
    for k in ("k_survey", "k_survey_reduce"):
        assert t[k]["spill"] == 0 and t[k]["scratch"] == 0, (k, t[k])
    assert t["k_survey"]["vgpr"] <= 512 and t["k_survey_reduce"]["vgpr"] <= 64, t      # (32 row values in flight per thread; up to 64 registers keep every wave slot)
    txt = (tmp_path / "survey.s").read_text()
    assert "scratch_" not in txt and "v_pk_fma_f32" not in txt and "v_fma_f32" not in txt      # no scratch instruction; products and sums rounded separately
    assert "global_atomic" not in txt and "flat_atomic" not in txt                               # the same pushes give the same bytes
