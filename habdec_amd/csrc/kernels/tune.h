// Per-stream digital tuning of the decimated chunk (hd_stream_set_tune / hd_stream_set_auto_afc, include/habdec_amd.h).
//
// Sample i of a call's chunk is multiplied by the phasor of theta = phase + i * step (mod 2^32, units of 2^-32 cycle).  The phasor is the product of two
// table entries, C[theta >> 24] = (cos, sin)(2 pi a / 256) and F[(theta >> 16) & 255] = (cos, sin)(2 pi b / 65536), each built once in double and rounded
// to float once.  Every complex product is (ur vr - ui vi, ur vi + ui vr) with each product and each sum rounded separately (the library is compiled with
// -ffp-contract=off; no fused multiply-add in either arithmetic mode), so the host restatement below and every kernel give the same bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define HD_TUNE_HD __host__ __device__ __forceinline__
#else
#define HD_TUNE_HD inline
#endif

namespace hd {

constexpr uint32_t kTuneTable = 256;   // entries per table; the tables sit back to back as [C | F], interleaved (cos, sin)

// (yr, yi) = (xr, xi) * (vr, vi), every operation rounded to float on its own
HD_TUNE_HD void tune_cmul(float xr, float xi, float vr, float vi, float& yr, float& yi)
{
    const float rr = xr * vr, ii = xi * vi, ri = xr * vi, ir = xi * vr;
    yr = rr - ii;
    yi = ri + ir;
}

// y = x * (C[a] * F[b]) for the two table entries of a sample's theta
HD_TUNE_HD void tune_apply(float cr, float ci, float fr, float fi, float xr, float xi, float& yr, float& yi)
{
    float pr, pi;
    tune_cmul(cr, ci, fr, fi, pr, pi);
    tune_cmul(xr, xi, pr, pi, yr, yi);
}

// Rotate one sample by theta; `tab` = [C | F] as 2 * kTuneTable (cos, sin) pairs.
HD_TUNE_HD void tune_rotate1(const float* tab, uint32_t theta, float xr, float xi, float& yr, float& yi)
{
    const uint32_t ia = theta >> 24, ib = (theta >> 16) & 255u;
    tune_apply(tab[2 * ia], tab[2 * ia + 1], tab[2 * (kTuneTable + ib)], tab[2 * (kTuneTable + ib) + 1], xr, xi, yr, yi);
}

}  // namespace hd
