// 4FSK tone tracker: the four-tone comb detector (hd_fsk4_track_*, include/habdec_amd.h has the definition in nine steps; host/fsk4_track.hpp restates this
// kernel step by step).  Not in the reference.
//
// k_fsk4_comb: one workgroup of 256 threads per stream, one launch for every stream whose epoch ended (src[s].due; the others' workgroups leave at once).
// A thread loads 16 of the stream's 4096 fftshifted double sums (bin t + 256 j: coalesced) and keeps them in registers to the end, where the decayed
// sums are stored back.  Steps 1 .. 3 are workgroup reductions over those registers: the finiteness test and the maximum, the quantisation (one IEEE
// double division per bin, -fno-fast-math), and the lower median by a bitwise select -- 20 rounds of "how many bins lie below this value", no sorting.
// q, its prefix sums and the window sums B[c] = sum of q over c - h .. c + h lie in LDS (48 KiB).  Step 5 spreads the candidates over the threads: the
// spacing d is the outer loop, alike in all threads, the lowest centre c0 the inner one, thread t taking c0 = first + t + 256 i -- neighbouring threads
// read neighbouring words of B, so the four reads of a candidate are free of bank conflicts.  A thread keeps its best (score, d, c0); the winner is a
// butterfly maximum over the packed key (score << 32 | 0xFFFF - d << 16 | 0xFFFF - c0) through the wave and the four waves' keys through LDS.  Steps 6 .. 9
// are a few hundred integer operations: threads 0 .. 3 refine a tone each, thread 0 fits the line and stores the record, 16 words.  Integer arithmetic
// behind the quantisation, no atomics, plain vector stores.
//
// Bounds: every index into q, ps and B follows from the plan's integers, which the kernel tests against the bounds the host guarantees
// (fsk4_track_state.hpp: Fsk4CombPlan) before it searches; a plan that fails them gives the all-zero record.
#include <hip/hip_runtime.h>

#include "fsk4_track.h"
#include "wave_util.h"

namespace hd {

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64, kBins = kFsk4CombBins, kPer = kBins / kThreads;
static_assert(kPer == 16, "a thread's 16 bins");

__device__ __forceinline__ uint32_t lane_xor(uint32_t v, uint32_t o) { return (uint32_t)__shfl_xor((int)v, (int)o, 64); }
__device__ __forceinline__ uint64_t lane_xor(uint64_t v, uint32_t o) { return ((uint64_t)lane_xor((uint32_t)(v >> 32), o) << 32) | lane_xor((uint32_t)v, o); }
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b)
{
    const int64_t q = a / b;
    return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

}  // namespace

__global__ __launch_bounds__(256) void k_fsk4_comb(const Fsk4CombSrc* __restrict__ src, double* acc_all, size_t acc_stride, uint32_t* rec_all, size_t rec_stride)
{
    __shared__ uint32_t q[kBins], ps[kBins + 4], B[kBins];
    __shared__ uint32_t part[2 * kWaves];
    __shared__ double dpart[kWaves];
    __shared__ unsigned long long kpart[kWaves];
    __shared__ int32_t cen[4];
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const Fsk4CombSrc d = src[s];
    if (!uni32(d.due)) return;                                       // the whole workgroup
    double* acc = acc_all + (size_t)s * acc_stride + kFsk4TrackGuard / 2;
    uint32_t* rec = rec_all + (size_t)s * rec_stride + kFsk4TrackGuard;
    const uint32_t w = uni32(d.plan.w), h = w / 2, d_lo = uni32(d.plan.d_lo), d_hi = uni32(d.plan.d_hi), b_lo = uni32(d.plan.b_lo), b_hi = uni32(d.plan.b_hi);
    const bool plan_ok = (w & 1u) && w >= 3u && w < kBins / 8u && d_lo >= 4u && d_lo <= d_hi && d_hi <= 4u * kBins && b_hi < kBins &&
                         (uint64_t)b_lo + 2u * h + ((3u * (uint64_t)d_hi + 2u) >> 2) <= b_hi;

    // ---- 1: the sums, their finiteness and their maximum
    double v[kPer];
    bool bad = false;
    double mx = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        v[j] = acc[t + kThreads * j];
        bad |= !__builtin_isfinite(v[j]);
        mx = v[j] > mx ? v[j] : mx;
    }
    for (uint32_t o = 32; o; o >>= 1) {
        const double other = __shfl_xor(mx, (int)o, 64);
        mx = other > mx ? other : mx;
    }
    if (lane == 0) dpart[wave] = mx;
    bad = __syncthreads_or(bad) != 0;                                // (a barrier: dpart is written)
    mx = fmax(fmax(dpart[0], dpart[1]), fmax(dpart[2], dpart[3]));
    const double keep = (double)uni32(d.decay_q8) / 256.0;
    if (bad || !(mx > 0.0) || !plan_ok) {
        if (t < 16u) rec[t] = 0u;
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) acc[t + kThreads * j] = v[j] * keep;
        return;
    }

    // ---- 2: quantisation
    uint32_t qv[kPer];
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        qv[j] = v[j] > 0.0 ? (uint32_t)floor(v[j] / mx * 524288.0) : 0u;
        q[t + kThreads * j] = qv[j];
    }

    // ---- 3: the lower median: the largest value with at most 2047 bins below it
    uint32_t floor_q = 0;
    for (int b = 19; b >= 0; --b) {
        const uint32_t trial = floor_q | (1u << b);
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) cnt += qv[j] < trial;
        for (uint32_t o = 32; o; o >>= 1) cnt += lane_xor(cnt, o);
        uint32_t* pp = part + (b & 1) * kWaves;                      // (two sets, alternated: one barrier a round)
        if (lane == 0) pp[wave] = cnt;
        __syncthreads();
        if (pp[0] + pp[1] + pp[2] + pp[3] <= kBins / 2 - 1) floor_q = trial;
    }

    // ---- prefix sums: thread t owns bins 16 t .. 16 t + 15 here
    {
        uint32_t own[kPer], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) { own[j] = q[kPer * t + j]; sum += own[j]; }
        const uint32_t incl = wave_scan(sum, lane);
        __syncthreads();                                             // (the last round's reads of part are done)
        if (lane == 63u) part[wave] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (uint32_t k = 0; k < wave; ++k) run += part[k];
        if (t == 0) ps[0] = 0u;
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) { run += own[j]; ps[kPer * t + j + 1u] = run; }
    }
    __syncthreads();
    // ---- 4: the window sums
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t c = t + kThreads * j;
        B[c] = c >= h && c + h < kBins ? ps[c + h + 1u] - ps[c - h] : 0u;
    }
    __syncthreads();

    // ---- 5: the coarse search
    uint32_t bs = 0, bd = 0, bc = 0;
    bool have = false;
    for (uint32_t dd = d_lo; dd <= d_hi; ++dd) {
        const uint32_t o1 = (dd + 2u) >> 2, o2 = (2u * dd + 2u) >> 2, o3 = (3u * dd + 2u) >> 2;
        const uint32_t last = b_hi - h - o3;                         // >= b_lo + h: plan_ok
        for (uint32_t c0 = b_lo + h + t; c0 <= last; c0 += kThreads) {
            const uint32_t sc = min(min(B[c0], B[c0 + o1]), min(B[c0 + o2], B[c0 + o3]));
            if (!have || sc > bs) { have = true; bs = sc; bd = dd; bc = c0; }          // (d and c0 ascend: the first of equals stays)
        }
    }
    uint64_t key = have ? (uint64_t)bs << 32 | (uint64_t)(0xFFFFu - bd) << 16 | (uint64_t)(0xFFFFu - bc) : 0ull;
    for (uint32_t o = 32; o; o >>= 1) {
        const uint64_t other = lane_xor(key, o);
        key = other > key ? other : key;
    }
    if (lane == 0) kpart[wave] = key;
    __syncthreads();
    key = kpart[0];
    for (uint32_t k = 1; k < kWaves; ++k) key = kpart[k] > key ? (uint64_t)kpart[k] : key;
    const uint32_t score = (uint32_t)(key >> 32), dbest = 0xFFFFu - (uint32_t)((key >> 16) & 0xFFFFu), c0best = 0xFFFFu - (uint32_t)(key & 0xFFFFu);

    // ---- 6: refinement, a tone per thread
    if (t < 4u) {
        int64_t c = (int64_t)c0best + ((t * dbest + 2u) >> 2), cf = 256 * c;
        for (int round = 0; round < 4; ++round) {
            int64_t sw = 0, sm = 0;
            const int64_t m0 = c - (int64_t)w > 0 ? c - (int64_t)w : 0, m1 = c + (int64_t)w < (int64_t)kBins - 1 ? c + (int64_t)w : (int64_t)kBins - 1;
            for (int64_t m = m0; m <= m1; ++m) {
                const uint32_t qm = q[m];
                const int64_t wt = qm > floor_q ? (int64_t)(qm - floor_q) : 0;
                sw += wt; sm += (m - c) * wt;
            }
            cf = 256 * c + (sw ? floor_div(512 * sm + sw, 2 * sw) : 0);
            c = (cf + 128) >> 8;                                     // (inside 0 .. 4095: a centroid of bins in that range)
        }
        cen[t] = (int32_t)cf;
    }
    __syncthreads();

    // ---- 7 .. 9: the fit, the quality, the record
    if (t == 0) {
        const int64_t c_0 = cen[0], c_1 = cen[1], c_2 = cen[2], c_3 = cen[3], sum = c_0 + c_1 + c_2 + c_3;
        int32_t spacing, f0;
        if (uni32(d.plan.known)) {
            spacing = (int32_t)(64u * dbest);
            f0 = (int32_t)floor_div(sum - 6 * (int64_t)spacing + 2, 4);
        } else {
            const int64_t s10 = -3 * c_0 - c_1 + c_2 + 3 * c_3;
            spacing = (int32_t)floor_div(s10 + 5, 10);
            f0 = (int32_t)floor_div(5 * sum - 3 * s10 + 10, 20);
        }
        const uint64_t wf = (uint64_t)w * floor_q;
        uint64_t quality = score > wf ? 256u * ((uint64_t)score - wf) / (wf ? wf : 1u) : 0u;
        if (quality > 0xFFFFFFFFull) quality = 0xFFFFFFFFull;
        const uint32_t valid = (uint32_t)quality >= uni32(d.min_quality_q8) && uni32(d.segments_ok) ? 1u : 0u;
        uint4* r4 = reinterpret_cast<uint4*>(rec);
        r4[0] = make_uint4((uint32_t)f0, (uint32_t)spacing, c0best, dbest);
        r4[1] = make_uint4(w, floor_q, score, (uint32_t)quality);
        r4[2] = make_uint4(valid, (uint32_t)cen[0], (uint32_t)cen[1], (uint32_t)cen[2]);
        r4[3] = make_uint4((uint32_t)cen[3], 0u, 0u, 0u);
    }

    // ---- the decay: one rounding per bin
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) acc[t + kThreads * j] = v[j] * keep;
}

void launch_fsk4_comb(hipStream_t st, uint32_t n_streams, const Fsk4CombSrc* src, double* acc, size_t acc_stride, uint32_t* rec, size_t rec_stride)
{
    hipLaunchKernelGGL(k_fsk4_comb, dim3(n_streams), dim3(kThreads), 0, st, src, acc, acc_stride, rec, rec_stride);
}

}  // namespace hd
