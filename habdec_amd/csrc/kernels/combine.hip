// Diversity combiner (hd_combine_*, include/habdec_amd.h has the definition; host/combine.hpp restates it sample by sample).  Not in the reference.
//
// k_combine: workgroups over (group, tile of 256 samples of the launch's chunk), one sample per thread.  A thread quantises its sample of every member,
// stores it into the member's int16 ring, fetches the member's delayed sample -- from the input row when it lies inside this push, from the ring when it
// is older -- and forms the weighted sum.  k_combine_lags: the sign-agreement scores of one member against the reference, 256 lags per workgroup, from
// 64-bit sign words in LDS; k_combine_lags_reduce: peak, tie rule and second peak of one member.  Integer arithmetic behind the quantisation, no atomics,
// plain vector stores.
//
// One arithmetic, like clocked.hip and tones.hip: not compiled per mode.
#include <hip/hip_runtime.h>

#include "combine.h"
#include "wave_util.h"

namespace hd {

namespace {

constexpr uint32_t kMask = kCombineRing - 1u;
constexpr uint32_t kMaxWords = HD_COMBINE_MAX_WINDOW / 64u;          // sign words of the longest window

// (the clocked decoder's rule, restated by the host's combine_quantise)
__device__ __forceinline__ int32_t quantise(float v)
{
    if (v != v) return 0;
    return (int32_t)(fminf(fmaxf(v, -4.0f), 4.0f) * 1024.0f);
}

// sample k of the push: linear memory, or the engine's symbol ring, where the push starts at `first`
__device__ __forceinline__ float load(const CombineSrc& d, uint32_t first, uint32_t k)
{
    return d.ring_mask ? d.p[(first + k) & d.ring_mask] : d.p[k];
}

struct LagArgs {
    uint64_t n;
    uint32_t N, L, guard, min_peak_q8, min_margin_q8, ref;
    uint32_t member[kCombineMembers - 1];
};

// a beats b: the larger score; ties go to the smaller |l|, then to the negative l
__device__ __forceinline__ bool beats(int32_t sa, int32_t la, int32_t sb, int32_t lb)
{
    if (sa != sb) return sa > sb;
    const int32_t aa = la < 0 ? -la : la, ab = lb < 0 ? -lb : lb;
    if (aa != ab) return aa < ab;
    return la < lb;
}

}  // namespace

__global__ __launch_bounds__(256) void k_combine(const CombineSrc* __restrict__ src, const CombineGroup* __restrict__ groups, int16_t* ring_all,
                                                 size_t ring_stride, float* rows, size_t row_stride, uint32_t row_cap)
{
    const CombineGroup* g = groups + blockIdx.x;
    const uint32_t count = min(uni32(g->count), kCombineMembers), r = uni32(g->stream[0]);
    const uint32_t n = min(uni32(src[r].n), (uint32_t)HD_COMBINE_CHUNK), off = uni32(src[r].off);      // (every member's n and off are the reference's: the host's check)
    const uint32_t j = blockIdx.y * kCombineTile + threadIdx.x;
    if (j >= n) return;
    const uint32_t k = off + j;                                      // the sample's index in the push
    const uint64_t i = uni64(g->base) + k;                           // ... and in the group since its last reset
    int32_t sum = 0;
    for (uint32_t m = 0; m < count; ++m) {
        const uint32_t s = uni32(g->stream[m]), dl = min(uni32(g->delay[m]), (uint32_t)HD_COMBINE_MAX_DELAY), w = uni32(g->weight[m]);
        const CombineSrc d = src[s];
        uint32_t first = 0;
        if (d.ring_mask) first = d.sym->base + d.sym->held - d.n_total;
        int16_t* ring = ring_all + (size_t)s * ring_stride + 2u * kCombineGuard;
        const int32_t q = quantise(load(d, first, k));
        // Ring slots read and written in one launch never coincide: the launch writes the indices [base + off, base + off + n) and reads indices in
        // [base + off - dl, base), and n + dl <= 4096 + 8192 < 32768.  (Reads never reach a sample of this push: those come from the input row.)
        ring[(uint32_t)i & kMask] = (int16_t)q;
        int32_t qd = q;
        if (dl) {
            if (i < dl) qd = 0;
            else if (k >= dl) qd = quantise(load(d, first, k - dl));
            else qd = ring[(uint32_t)(i - dl) & kMask];
        }
        sum += (int32_t)w * qd;
    }
    const int32_t o = sum / (int32_t)max(uni32(g->wt), 1u);         // truncated toward zero
    if (k < row_cap) rows[(size_t)r * row_stride + kCombineGuard + k] = (float)o / 1024.0f;
}

// Grid (member, block of 256 lag indices).  Lag index a = l + L, 0 .. 2 L.  The reference's window is the samples [n - L - N, n - L); at lag index a the
// member's window starts a samples behind n - N - 2 L.  Lags of consecutive lanes are consecutive and a wave's 64 lags start on a word boundary, so the
// lanes of a wave differ in the shift only: both LDS reads of the inner loop are one address per wave (a broadcast, no bank is asked twice), and the four
// waves are one word apart.
__global__ __launch_bounds__(256) void k_combine_lags(LagArgs a, const int16_t* __restrict__ ring_all, size_t ring_stride, int32_t* __restrict__ scores)
{
    __shared__ unsigned long long R[kMaxWords];
    __shared__ unsigned long long M[kMaxWords + kCombineLagBlock / 64u + 1u];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t N = min(a.N, (uint32_t)HD_COMBINE_MAX_WINDOW), L = min(a.L, (uint32_t)HD_COMBINE_MAX_LAG), nw = N / 64u;
    const uint32_t a0 = blockIdx.y * kCombineLagBlock;
    const int16_t* rr = ring_all + (size_t)a.ref * ring_stride + 2u * kCombineGuard;
    const int16_t* rm = ring_all + (size_t)a.member[blockIdx.x] * ring_stride + 2u * kCombineGuard;
    const uint64_t r0 = a.n - L - N, m0 = a.n - N - 2u * L + a0;
    for (uint32_t w = wave; w < nw; w += 4u)
        R[w] = __ballot(rr[(uint32_t)(r0 + 64u * w + lane) & kMask] > 0);
    for (uint32_t w = wave; w < nw + kCombineLagBlock / 64u + 1u; w += 4u) {
        const uint64_t i = m0 + 64u * w + lane;                      // (behind the member's last sample in the last block only: no live lag reads those bits)
        M[w] = __ballot(i < a.n && rm[(uint32_t)i & kMask] > 0);
    }
    __syncthreads();
    if (a0 + t > 2u * L) return;
    uint32_t agree = 0;
    unsigned long long lo = M[wave];
    for (uint32_t j = 0; j < nw; ++j) {
        const unsigned long long hi = M[wave + j + 1u];
        const unsigned long long x = lane ? (lo >> lane) | (hi << (64u - lane)) : lo;
        agree += (uint32_t)__popcll(~(R[j] ^ x));
        lo = hi;
    }
    scores[(size_t)blockIdx.x * (2u * L + 1u) + a0 + t] = 2 * (int32_t)agree - (int32_t)N;
}

// One workgroup per member: lag and peak by the tie rule, then `second`, the largest score more than `guard` lags away from the peak.
__global__ __launch_bounds__(256) void k_combine_lags_reduce(LagArgs a, const int32_t* __restrict__ scores, hd_combine_lag* __restrict__ out)
{
    __shared__ int32_t best_s[256], best_l[256];
    const uint32_t t = threadIdx.x;
    const int32_t L = (int32_t)min(a.L, (uint32_t)HD_COMBINE_MAX_LAG), N = (int32_t)a.N;
    const int32_t* sc = scores + (size_t)blockIdx.x * (2u * (uint32_t)L + 1u);
    int32_t bs = -N - 1, bl = 0;                                     // (below every score)
    for (int32_t k = (int32_t)t; k <= 2 * L; k += 256) {
        const int32_t s = sc[k], l = k - L;
        if (beats(s, l, bs, bl)) { bs = s; bl = l; }
    }
    best_s[t] = bs; best_l[t] = bl;
    __syncthreads();
    for (uint32_t h = 128u; h; h >>= 1) {
        if (t < h && beats(best_s[t + h], best_l[t + h], best_s[t], best_l[t])) { best_s[t] = best_s[t + h]; best_l[t] = best_l[t + h]; }
        __syncthreads();
    }
    const int32_t peak = best_s[0], lag = best_l[0];
    __syncthreads();
    int32_t second = -N;                                             // (no lag that far away: the least score there is)
    for (int32_t k = (int32_t)t; k <= 2 * L; k += 256) {
        const int32_t d = k - L - lag;
        if ((uint32_t)(d < 0 ? -d : d) > a.guard) second = max(second, sc[k]);
    }
    best_s[t] = second;
    __syncthreads();
    for (uint32_t h = 128u; h; h >>= 1) {
        if (t < h) best_s[t] = max(best_s[t], best_s[t + h]);
        __syncthreads();
    }
    if (t == 0) {
        second = best_s[0];
        hd_combine_lag o;
        o.stream = a.member[blockIdx.x]; o.lag = lag; o.peak = peak; o.second = second;
        o.valid = (256ll * peak >= (long long)a.min_peak_q8 * N && 256ll * ((long long)peak - second) >= (long long)a.min_margin_q8 * N) ? 1u : 0u;
        out[blockIdx.x] = o;
    }
}

void launch_combine(hipStream_t st, uint32_t n_groups, uint32_t cap, const CombineSrc* src, const CombineGroup* groups, int16_t* ring, size_t ring_stride,
                    float* rows, size_t row_stride, uint32_t row_cap)
{
    if (!n_groups || !cap) return;
    hipLaunchKernelGGL(k_combine, dim3(n_groups, (cap + kCombineTile - 1u) / kCombineTile), dim3(kCombineTile), 0, st, src, groups, ring, ring_stride, rows,
                       row_stride, row_cap);
}

void launch_combine_lags(hipStream_t st, const CombineGroup* group, uint64_t n, uint32_t N, uint32_t L, uint32_t guard, uint32_t min_peak_q8,
                         uint32_t min_margin_q8, const int16_t* ring, size_t ring_stride, int32_t* scores, hd_combine_lag* out)
{
    if (group->count < 2u) return;
    LagArgs a{};
    a.n = n; a.N = N; a.L = L; a.guard = guard; a.min_peak_q8 = min_peak_q8; a.min_margin_q8 = min_margin_q8; a.ref = group->stream[0];
    for (uint32_t m = 1; m < group->count; ++m) a.member[m - 1] = group->stream[m];
    hipLaunchKernelGGL(k_combine_lags, dim3(group->count - 1u, (2u * L + 1u + kCombineLagBlock - 1u) / kCombineLagBlock), dim3(kCombineLagBlock), 0, st, a,
                       ring, ring_stride, scores);
    hipLaunchKernelGGL(k_combine_lags_reduce, dim3(group->count - 1u), dim3(256), 0, st, a, scores, out);
}

}  // namespace hd
