// Tone search: a Welch-averaged power spectrum per stream at the decimated rate, kept over many pushes (hd_tone_search_*, include/habdec_amd.h).  Not in
// the reference: its only per-decoder spectrum is one 4096-sample snapshot (Decoder.h:467-520), whose peaks the AFC misjudges on a weak signal.
//
// k_tone_search: one wave per stream, the mapping of k_survey -- 64 registers of samples per lane, one wave per SIMD.  A stream's segments are cut over
// its absolute sample index, so they straddle pushes: the wave reads each newly completed segment from the logical concatenation [carry | row] (a select
// per load), windows and transforms it exactly as k_survey does (the same float table, specwave::fft64 and finish4096 with the same twiddle schedule),
// and adds |X|^2 of every bin, fftshifted, into the stream's double accumulator itself, segment by segment.  No float sums across segments and no
// atomics: the accumulator's bytes depend on the stream's samples alone, not on how they were cut into pushes or launches.
//
// The carry: two buffers per stream, alternated.  A launch that completes a segment writes the new carry -- the samples from 2048 segs on -- into the
// OTHER buffer, so nothing it still has to read is ever overwritten and no argument about the order of one wave's loads and stores is needed; a launch
// that completes none appends its samples behind the old carry in place, which overwrites nothing.  The price is 32 KiB per stream.
//
// One arithmetic, like survey.hip: every product and sum is rounded separately (-ffp-contract=off); not compiled per arithmetic mode.
#include <hip/hip_runtime.h>

#include "spectrum_wave.h"
#include "tone_search.h"
#include "wave_util.h"

namespace hd {

static_assert(kToneSearchSeg == (uint32_t)kFftBins, "the tone search uses the engine's 4096-point transform and twiddles");

namespace {

typedef __attribute__((address_space(1))) double* gdouble_t;
typedef const __attribute__((address_space(1))) float* gfloat_t;

// sample g of [carry | row]: both are device memory on every route
__device__ __forceinline__ f32x2 cat_load(const float2* cin, const float2* row, const uint32_t c, const uint32_t g)
{
    const float2* q = g < c ? cin + g : row + (g - c);
    return *(specwave::gptr_t)q;
}

}  // namespace

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_tone_search(const ToneSearchSrc* __restrict__ src,
                                                                                               const float* __restrict__ win,
                                                                                               const float2* __restrict__ tw64, double* acc_all,
                                                                                               const size_t acc_stride, float2* carry_all,
                                                                                               const size_t carry_stride)
{
    __shared__ float plane[64 * 65];
    const uint32_t l = threadIdx.x & 63u, s = blockIdx.x;
    const ToneSearchSrc d = src[s];
    const uint32_t n = uni32(d.n), c = uni32(d.carry), segs = uni32(d.segs), flip = uni32(d.flip) & 1u;
    if (!n) return;                                                  // nothing of this stream in this launch
    const float2* row = d.p + uni32(d.off);
    float2* const cbuf = carry_all + (size_t)s * 2 * carry_stride + kToneSearchGuard / 2;
    const float2* cin = cbuf + flip * carry_stride;
    float2* cout = cbuf + (segs ? flip ^ 1u : flip) * carry_stride;
    double* acc = acc_all + (size_t)s * acc_stride + kToneSearchGuard / 2;
    for (uint32_t j = 0; j < segs; ++j) {
        const uint32_t base = j * kToneSearchStep + l;
        // (the table's and the sums' bases become this iteration's own values: hoisted out of the loop, the row bases derived from them would hold more
        // scalar registers for the whole loop than a wave has beside the transform's constants)
        const float* winj = win;
        double* accj = acc;
        asm volatile("" : "+s"(winj), "+s"(accj));
        // (device memory: said so behind the opaque base, or the loads would be flat ones.  k_survey reads the table through its kernel
        // argument, whose address space the compiler knows: the window loop below is k_survey's but for this pointer type, so the two stay apart.)
        const gfloat_t win1 = (gfloat_t)winj;
        f32x2 a[64];
        // ---- pass 1 input: lane n2 = l takes x[64 n1 + l] w[64 n1 + l], x from the carry or the row; all 64 loads go out before the first product
        // (eight at a time: the scheduler would otherwise form all 64 compare masks first, more scalar registers than a wave has)
#pragma unroll
        for (int g = 0; g < 64; g += 8) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 8; ++u) a[g + u] = cat_load(cin, row, c, base + 64 * (g + u));
        }
        uint32_t wl = l;
        asm volatile("" : "+v"(wl));
#pragma unroll
        for (int g = 0; g < 64; g += 16) {
            __builtin_amdgcn_sched_barrier(0);
            float wv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) wv[u] = win1[64 * (g + u) + wl];
#pragma unroll
            for (int u = 0; u < 16; ++u) a[g + u] = (f32x2){a[g + u].x * wv[u], a[g + u].y * wv[u]};
        }
        f32x2 w[64];
        specwave::load_tw(w, tw64, 0, kTwSoloH, l);
        specwave::fft64(a);
        specwave::finish4096<kTwSoloG, kTwSoloH, kTwSoloD>(a, w, tw64, plane, l);                // a[xpos(k2)] = X[l + 64 k2]
        // ---- half swap and accumulation: bin k = l + 64 k2 lands at i = (k + 2048) & 4095 = l + 64 jj, jj = (k2 + 32) & 63.  Every lane owns its 64 sums:
        // the next segment's loads of them follow this one's stores in the same lane.
#pragma unroll
        for (int g = 0; g < 64; g += 8) {
            __builtin_amdgcn_sched_barrier(0);
            double* ag = accj + 64 * g;
            asm volatile("" : "+s"(ag));
            const gdouble_t ag1 = (gdouble_t)ag;                   // (device memory: said so behind the opaque base, or these would be flat accesses)
            double t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = ag1[64 * u + l];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const f32x2 v = a[specwave::xpos((g + u + 32) & 63)];
                const float p = v.x * v.x + v.y * v.y;
                ag1[64 * u + l] = t[u] + (double)p;
            }
        }
    }
    // ---- the carry: samples [2048 segs, c + n) of [carry | row]; with segs = 0 the first c of them are where they belong already
    const uint32_t sh = segs * kToneSearchStep, m = c + n - sh;
    for (uint32_t i = (segs ? 0u : c) + l; i < m; i += 64) {
        const f32x2 v = cat_load(cin, row, c, i + sh);
        cout[i] = make_float2(v.x, v.y);
    }
}

void launch_tone_search(hipStream_t st, uint32_t n_streams, const ToneSearchSrc* src, const float* win, const float2* tw64, double* acc, size_t acc_stride,
                        float2* carry, size_t carry_stride)
{
    hipLaunchKernelGGL(k_tone_search, dim3(n_streams), dim3(64), 0, st, src, win, tw64, acc, acc_stride, carry, carry_stride);
}

}  // namespace hd
