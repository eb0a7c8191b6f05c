// Wideband survey: a Welch-averaged power spectrum of full-rate IQ (hd_survey_*, include/habdec_amd.h).  Not in the reference: its spectrum is per
// decoder at the decimated rate (Decoder.h:467-520), so it sees +-fs_dec/2 around an offset that is already known.
//
// k_survey: one wave per run of consecutive 4096-sample segments (hop 2048).  Per segment: window (periodic Hann, a float table), the in-wave
// 64 x 64 transform of spectrum_wave.h -- the same load layout as spectrum_wave_body, and its twiddles, transpose and second pass
// (specwave::finish4096) --, then |X|^2 of the lane's 64 bins added into 64 float accumulators that live in registers for the whole run.
// The run's row goes out fftshifted.  k_survey_reduce adds the rows of a launch, in run order, into the survey's double accumulators.
// No atomics: which sums are formed depends on the push's length alone, so the same pushes give the same bytes.
//
// One arithmetic: every product and sum is rounded separately (-ffp-contract=off) and the result is compared norm-wise, so this file is not
// compiled per arithmetic mode.
#include <hip/hip_runtime.h>

#include "spectrum_wave.h"
#include "survey.h"

namespace hd {

static_assert(kSurveyBins == (uint32_t)kFftBins, "the survey uses the engine's 4096-point transform and twiddles");

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_survey(const float2* __restrict__ x, const float* __restrict__ win,
                                                                                          const float2* __restrict__ tw64, float* __restrict__ partial,
                                                                                          const uint64_t seg0, const uint64_t n_seg, const uint32_t run_len)
{
    __shared__ float plane[64 * 65];
    const uint32_t l = threadIdx.x & 63u;
    const uint64_t first = seg0 + (uint64_t)blockIdx.x * run_len;
    const uint64_t last = first + run_len < n_seg ? first + run_len : n_seg;
    float acc[64];                                                  // acc[i] belongs to the bin register a[i] holds after pass 2: X[l + 64 k2] at i = xpos(k2)
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = 0.0f;
    for (uint64_t s = first; s < last; ++s) {
        const float2* xs = x + s * kSurveyHop;
        f32x2 a[64];
        // ---- pass 1 input: lane n2 = l takes x[64 n1 + l] w[64 n1 + l].  All 64 sample loads of the segment are issued before the first product: with one
        // wave per SIMD (the accumulators' price) nothing else hides their latency.  The window comes through the cache, sixteen rows at a time, behind a
        // lane offset the compiler cannot see through: hoisted out of the segment loop its 64 values would not fit beside a[] and acc[].
#pragma unroll
        for (int n1 = 0; n1 < 64; ++n1) { const float2 v = xs[64 * n1 + l]; a[n1] = (f32x2){v.x, v.y}; }
        uint32_t wl = l;
        asm volatile("" : "+v"(wl));
#pragma unroll
        for (int g = 0; g < 64; g += 16) {
            __builtin_amdgcn_sched_barrier(0);
            float wv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) wv[u] = win[64 * (g + u) + wl];
#pragma unroll
            for (int u = 0; u < 16; ++u) a[g + u] = (f32x2){a[g + u].x * wv[u], a[g + u].y * wv[u]};
        }
        f32x2 w[64];
        specwave::load_tw(w, tw64, 0, kTwSoloH, l);                    // (the first twiddle rows, in front of pass 1)
        specwave::fft64(a);
        specwave::finish4096<kTwSoloG, kTwSoloH, kTwSoloD>(a, w, tw64, plane, l);                // twiddle, transpose, pass 2: a[xpos(k2)] = X[l + 64 k2]
#pragma unroll
        for (int i = 0; i < 64; ++i) acc[i] = acc[i] + (a[i].x * a[i].x + a[i].y * a[i].y);
    }
    // ---- half swap: bin k = l + 64 k2 lands at i = (k + 2048) & 4095 = l + 64 j, j = (k2 + 32) & 63; wave-wide contiguous stores
    float* row = partial + (size_t)blockIdx.x * kSurveyBins;
#pragma unroll
    for (int g = 0; g < 64; g += 8) {
        float* rg = row + 64 * g;
        asm volatile("" : "+s"(rg));
#pragma unroll
        for (int u = 0; u < 8; ++u) rg[64 * u + l] = acc[specwave::xpos((g + u + 32) & 63)];
    }
}

// 4096 threads for a launch's rows (16 MB at 1024 runs): 64 waves cannot hide a load's latency by number, so each thread keeps 32 row loads in flight
// and then adds them in run order -- the order of the additions is what the result depends on, not the order of the loads.
__global__ __launch_bounds__(256) void k_survey_reduce(const float* __restrict__ partial, const uint32_t n_runs, double* __restrict__ acc)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;             // the grid is exactly kSurveyBins threads
    const float* p = partial + i;
    double v = acc[i];
    uint32_t r = 0;
    for (; r + 32 <= n_runs; r += 32) {
        float t[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) t[u] = p[(size_t)(r + u) * kSurveyBins];
#pragma unroll
        for (int u = 0; u < 32; ++u) v += (double)t[u];
    }
    for (; r < n_runs; ++r) v += (double)p[(size_t)r * kSurveyBins];
    acc[i] = v;
}

void launch_survey(hipStream_t st, uint32_t n_runs, const float2* x, const float* win, const float2* tw64, float* partial, uint64_t seg0, uint64_t n_seg,
                   uint32_t run_len)
{
    hipLaunchKernelGGL(k_survey, dim3(n_runs), dim3(64), 0, st, x, win, tw64, partial, seg0, n_seg, run_len);
}

void launch_survey_reduce(hipStream_t st, const float* partial, uint32_t n_runs, double* acc)
{
    hipLaunchKernelGGL(k_survey_reduce, dim3(kSurveyBins / 256), dim3(256), 0, st, partial, n_runs, acc);
}

}  // namespace hd
