// Tone-filter demodulator (hd_tones_*, include/habdec_amd.h has the definition; host/tones.hpp restates it sample by sample).  Not in the reference.
//
// k_tones: one workgroup of 256 threads per stream, one launch per chunk of at most HD_TONES_CHUNK samples.  A stream's history is kept as running sums
// (host/tones_state.hpp): the four rotation sums mod 2^32, the normaliser's mod 2^64.  The chunk goes through in tiles of 256 samples, one per thread: a
// thread quantises its sample and turns it against both tones, a workgroup scan (wave scan, then the waves' totals through LDS) makes the running sums,
// which stay in LDS for the whole chunk.  A lagged sum comes from LDS when it lies inside the chunk and from the stream's ring in device memory when it
// is older; the rings are only read until the last tile is done, then the chunk's newest sums are stored over the oldest.  Integer arithmetic behind the
// quantisation, no atomics, plain vector stores.
//
// One arithmetic, like baud_probe.hip and clocked.hip: not compiled per mode.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "wave_util.h"

namespace hd {

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;

// LDS of a launch whose longest row has `cap` samples: Q[cap1] uint64 | P[4][cap1] uint32 | C[1024] | the waves' totals; every part a multiple of 16 bytes
__host__ __device__ __forceinline__ uint32_t lds_cap1(uint32_t cap) { return (cap + 1u + 3u) & ~3u; }
__host__ __device__ __forceinline__ uint32_t lds_bytes(uint32_t cap) { return lds_cap1(cap) * 24u + 1024u * 4u + 4u * kWaves * 4u + kWaves * 8u; }

// (its own range and scale, restated by the host's tones_quantise: not to be merged with clocked.hip's, see there)
__device__ __forceinline__ int32_t quantise(float v)
{
    if (v != v) return 0;
    return (int32_t)(fminf(fmaxf(v, -8.0f), 8.0f) * 256.0f);
}

// floor(sqrt(x)), x < 2^48: the float estimate is a few units off at most, integer comparisons settle it
__device__ __forceinline__ uint32_t isqrt(uint64_t x)
{
    uint64_t r = (uint64_t)sqrtf((float)x);
    while (r * r > x) --r;
    while ((r + 1u) * (r + 1u) <= x) ++r;
    return (uint32_t)r;
}

}  // namespace

__global__ __launch_bounds__(256) void k_tones(const TonesSrc* __restrict__ src, TonesState* __restrict__ state, uint32_t* ring32_all, size_t ring32_stride,
                                               unsigned long long* ring64_all, size_t ring64_stride, const int32_t* __restrict__ ctab, float* rows,
                                               size_t row_stride, uint32_t row_cap, uint32_t cap)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    TonesState* st = state + s;
    const uint32_t F = uni32(st->F);
    const TonesSrc d = src[s];
    const uint32_t m = min(uni32(d.n), cap), off = uni32(d.off);
    if (!F || !m) return;                                            // no modem, or nothing of this stream in this launch (the whole workgroup)
    const uint32_t cap1 = lds_cap1(cap);
    unsigned long long* Q = reinterpret_cast<unsigned long long*>(smem);            // Q[j]: qtot after n + j samples
    uint32_t* P = reinterpret_cast<uint32_t*>(smem + (size_t)cap1 * 8u);              // P[k * cap1 + j]: tot[k] after n + j samples
    int32_t* C = reinterpret_cast<int32_t*>(smem + (size_t)cap1 * 24u);
    uint32_t* part32 = reinterpret_cast<uint32_t*>(C + 1024);                         // [4][kWaves]
    unsigned long long* part64 = reinterpret_cast<unsigned long long*>(part32 + 4u * kWaves);

    const uint32_t W = uni32(st->W), L = uni32(st->L), phi_hi = uni32(st->phi[0]), phi_lo = uni32(st->phi[1]);
    const uint64_t n = uni64(st->n);
    uint32_t carry[4];
    for (uint32_t k = 0; k < 4u; ++k) carry[k] = uni32(st->tot[k]);
    uint64_t qcarry = uni64(st->qtot);
    const uint32_t* ring32 = ring32_all + (size_t)s * 4u * ring32_stride + kTonesGuard;          // ring k: + k * ring32_stride
    const unsigned long long* ring64 = ring64_all + (size_t)s * ring64_stride + kTonesGuard / 2u;
    float* row = rows + (size_t)s * row_stride + kTonesGuard;

    for (uint32_t a = t; a < 1024u; a += kThreads) C[a] = ctab[a];
    if (t == 0) {
        for (uint32_t k = 0; k < 4u; ++k) P[k * cap1] = carry[k];
        Q[0] = qcarry;
    }
    __syncthreads();

    for (uint32_t base = 0; base < m; base += kThreads) {
        const uint32_t j = base + t;
        const bool live = j < m;
        // ---- quantise, rotate, running sums of the tile
        int32_t q_re = 0, q_im = 0;
        if (live) {
            const float2 v = d.p[off + j];
            q_re = quantise(v.x); q_im = quantise(v.y);
        }
        const uint32_t i32 = (uint32_t)n + j;                        // theta needs i mod 2^32 only
        uint32_t sum[4];
        {
            const uint32_t a_hi = (i32 * phi_hi) >> 22, a_lo = (i32 * phi_lo) >> 22;
            const int32_t c_hi = C[a_hi], s_hi = C[(a_hi + 768u) & 1023u], c_lo = C[a_lo], s_lo = C[(a_lo + 768u) & 1023u];
            sum[0] = (uint32_t)((q_re * c_hi + q_im * s_hi) >> 15);
            sum[1] = (uint32_t)((q_im * c_hi - q_re * s_hi) >> 15);
            sum[2] = (uint32_t)((q_re * c_lo + q_im * s_lo) >> 15);
            sum[3] = (uint32_t)((q_im * c_lo - q_re * s_lo) >> 15);
        }
        for (uint32_t k = 0; k < 4u; ++k) {
            sum[k] = wave_scan(sum[k], lane);
            if (lane == 63u) part32[k * kWaves + wave] = sum[k];
        }
        __syncthreads();
        for (uint32_t k = 0; k < 4u; ++k) {
            uint32_t before = carry[k], all = carry[k];
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t p = part32[k * kWaves + w];
                if (w < wave) before += p;
                all += p;
            }
            if (live) P[k * cap1 + j + 1u] = before + sum[k];
            carry[k] = all;
        }
        __syncthreads();
        // ---- windows, envelopes, the normaliser's running sum
        int32_t diff = 0;
        uint64_t tsum = 0;
        if (live) {
            int32_t w[4];
            const bool from_lds = j + 1u >= W, none = n + j + 1u <= W;              // the lagged index lies in the chunk / in front of index 0
            for (uint32_t k = 0; k < 4u; ++k) {
                uint32_t lag = 0;
                if (from_lds) lag = P[k * cap1 + j + 1u - W];
                else if (!none) lag = ring32[k * ring32_stride + ((uint32_t)(n + j + 1u - W) & (kTonesRing32 - 1u))];
                w[k] = (int32_t)(P[k * cap1 + j + 1u] - lag);
            }
            const uint32_t A_hi = isqrt((uint64_t)((int64_t)w[0] * w[0] + (int64_t)w[1] * w[1]));
            const uint32_t A_lo = isqrt((uint64_t)((int64_t)w[2] * w[2] + (int64_t)w[3] * w[3]));
            diff = (int32_t)A_hi - (int32_t)A_lo;
            tsum = (uint64_t)A_hi + A_lo;
        }
        tsum = wave_scan(tsum, lane);
        if (lane == 63u) part64[wave] = tsum;
        __syncthreads();
        {
            uint64_t before = qcarry, all = qcarry;
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint64_t p = part64[w];
                if (w < wave) before += p;
                all += p;
            }
            if (live) Q[j + 1u] = before + tsum;
            qcarry = all;
        }
        __syncthreads();
        // ---- output
        if (live) {
            uint64_t lag = 0;
            if (j + 1u >= L) lag = Q[j + 1u - L];
            else if (n + j + 1u > L) lag = ring64[(uint32_t)(n + j + 1u - L) & (kTonesRing64 - 1u)];
            const int64_t N = (int64_t)(Q[j + 1u] - lag);
            int64_t o = ((int64_t)diff * 1024 * (int64_t)L) / (N > 1 ? N : 1);
            o = o > 4096 ? 4096 : o < -4096 ? -4096 : o;
            if (off + j < row_cap) row[off + j] = (float)(int32_t)o / 1024.0f;
        }
    }
    __syncthreads();                                                 // every lagged value has been read: the chunk's newest sums go over the oldest
    {
        uint32_t* r32 = ring32_all + (size_t)s * 4u * ring32_stride + kTonesGuard;
        unsigned long long* r64 = ring64_all + (size_t)s * ring64_stride + kTonesGuard / 2u;
        for (uint32_t j = (m > kTonesRing32 ? m - kTonesRing32 : 0u) + t; j < m; j += kThreads)
            for (uint32_t k = 0; k < 4u; ++k) r32[k * ring32_stride + ((uint32_t)(n + j + 1u) & (kTonesRing32 - 1u))] = P[k * cap1 + j + 1u];
        for (uint32_t j = (m > kTonesRing64 ? m - kTonesRing64 : 0u) + t; j < m; j += kThreads)
            r64[(uint32_t)(n + j + 1u) & (kTonesRing64 - 1u)] = Q[j + 1u];
    }
    if (t == 0) {
        st->n = n + m; st->qtot = qcarry;
        for (uint32_t k = 0; k < 4u; ++k) st->tot[k] = carry[k];
    }
}

bool launch_tones(hipStream_t st, uint32_t n_streams, uint32_t cap, const TonesSrc* src, TonesState* state, uint32_t* ring32, size_t ring32_stride,
                  unsigned long long* ring64, size_t ring64_stride, const int32_t* ctab, float* rows, size_t row_stride, uint32_t row_cap)
{
    if (!cap || cap > HD_TONES_CHUNK) return false;
    const uint32_t bytes = lds_bytes(cap);
    if (bytes > 160u * 1024u) return false;
    if (bytes > 64u * 1024u && hipFuncSetAttribute(reinterpret_cast<const void*>(k_tones), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return false;
    hipLaunchKernelGGL(k_tones, dim3(n_streams), dim3(kThreads), bytes, st, src, state, ring32, ring32_stride, ring64, ring64_stride, ctab, rows, row_stride,
                       row_cap, cap);
    return true;
}

}  // namespace hd
