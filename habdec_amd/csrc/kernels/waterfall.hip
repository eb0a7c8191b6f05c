// Waterfall: the survey's float rows kept over time, and the detector run on every row on the GPU (hd_waterfall_*, include/habdec_amd.h).  Not in the
// reference.  The rows themselves are k_survey's (kernels/survey.hip, run_len = slot_segments, written straight into the ring); this file holds what
// turns a row into 16 bytes of results and 4096 mark bits, and the per-bin hit counters.
//
// k_waterfall_detect: one workgroup of 256 threads per row.  The row comes in with 16-byte loads per lane and goes through LDS once, which turns that
// layout into the one the ballots need: wave w, step j, lane l holds bin 1024 w + 64 j + l, so one ballot is two whole mark words.  The keys stay in 16
// registers per thread from there on.  The median of the eligible bins is a radix select over the keys read as unsigned integers (the order of the floats
// the pattern check admits): four passes of one byte each, a 256-bin histogram per wave in LDS (integer LDS atomics), the bin that holds the wanted rank
// found by one wave with a shuffle scan.  For an even count the lower middle value is the selected key itself when the rank lies inside its run of
// equals, else the largest key below it.  A sort would do 78 compare-exchange stages over 16 KB of LDS with strides that fold onto the same banks; the
// select reads the row out of LDS once and its atomics hit 1 KB per wave.
// k_waterfall_hits: one thread per bin and 64 rows adds the rows' mark bits and hands its count to the bin's counter with one integer atomic.
//
// Float operations are rounded once each (-ffp-contract=off): 0.5f * (a + b) and floor * factor, nothing else.  No floating-point atomics (the only
// global atomic is the hit counters' integer add), no scratch.
#include <hip/hip_runtime.h>

#include "habdec_amd.h"
#include "waterfall.h"

namespace hd {

static_assert(kWaterfallBins == HD_SURVEY_BINS && kWaterfallWords == HD_WATERFALL_WORDS && kWaterfallMaxSeg == HD_SURVEY_RUN, "the header's numbers");

constexpr uint32_t kWfThreads = 256;           // four waves: 1024 bins, 16 keys per lane, 32 mark words per wave
constexpr uint32_t kWfInf = 0x7F800000u;       // patterns above it are NaNs or carry a sign bit

__global__ __launch_bounds__(kWfThreads) void k_waterfall_detect(const float* __restrict__ rows, const uint32_t* __restrict__ segments, const uint32_t seg_full,
                                                                 const uint32_t seg_last, const uint32_t guard_lo, const uint32_t guard_hi,
                                                                 const float* __restrict__ factor, WaterfallRec* __restrict__ out)
{
    __shared__ uint32_t keys[kWaterfallBins];
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t sel[2];                 // the pass's bin and the rank left inside it
    __shared__ uint32_t wmax[4], wsum[4];
    const uint32_t t = threadIdx.x, l = t & 63u, w = t >> 6;
    const uint32_t seg = segments ? segments[blockIdx.x] : (blockIdx.x + 1 == gridDim.x ? seg_last : seg_full);
    WaterfallRec* rec = out + blockIdx.x;

    // ---- the row: 4 x 16 bytes per thread, consecutive threads consecutive addresses; LDS takes them at the same index
    const uint4* src = reinterpret_cast<const uint4*>(rows + (size_t)blockIdx.x * kWaterfallBins);
    uint4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = src[t + kWfThreads * j];
#pragma unroll
    for (int j = 0; j < 4; ++j) reinterpret_cast<uint4*>(keys)[t + kWfThreads * j] = v[j];
    __syncthreads();
    uint32_t k[16];
    uint32_t elig = 0;                          // bit j: bin 1024 w + 64 j + l is eligible
    int bad = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t i = 1024u * w + 64u * j + l;
        k[j] = keys[i];                         // (consecutive lanes, consecutive banks)
        bad |= k[j] > kWfInf;
        elig |= (uint32_t)(i < guard_lo || i >= guard_hi) << j;
    }
    uint32_t flags = seg < 16u ? HD_WF_SHORT : 0u;
    float floor = 0.0f, level = 0.0f;
    if (__syncthreads_or(bad)) {                // (the same answer in every thread: the barriers below are reached by all or by none)
        flags |= HD_WF_BAD;
    } else {
        // ---- radix select of s[m / 2] among the eligible keys, most significant byte first
        const uint32_t m = kWaterfallBins - (guard_hi - guard_lo);
        uint32_t prefix = 0, mask = 0, rank = m >> 1;
        for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
            for (int c = 0; c < 4; ++c) hist[c][t] = 0;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (((elig >> j) & 1u) && (k[j] & mask) == prefix) atomicAdd(&hist[w][(k[j] >> shift) & 255u], 1u);
            __syncthreads();
            if (w == 0) {                       // lane l: bins 4 l .. 4 l + 3, summed over the waves' histograms; an inclusive scan over the lanes
                uint32_t c[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) c[u] = hist[0][4 * l + u] + hist[1][4 * l + u] + hist[2][4 * l + u] + hist[3][4 * l + u];
                const uint32_t s = c[0] + c[1] + c[2] + c[3];
                uint32_t incl = s;              // (wave_util.h's wave_scan, written out: see there)
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(incl, d, 64);
                    if (l >= (uint32_t)d) incl += up;
                }
                const uint32_t excl = incl - s;
                if (rank >= excl && rank < incl) {          // exactly one lane: rank < the keys still in play
                    uint32_t r = rank - excl, b = 4 * l;
#pragma unroll
                    for (int u = 0; u < 3; ++u)
                        if (b == 4 * l + u && r >= c[u]) { r -= c[u]; ++b; }
                    sel[0] = b; sel[1] = r;
                }
            }
            __syncthreads();
            prefix |= sel[0] << shift;
            mask |= 255u << shift;
            rank = sel[1];                      // (sel is written again two barriers from here)
        }
        // ---- prefix = s[m / 2]; rank = how many equal keys stand in front of it.  The largest eligible key below it, should s[m / 2 - 1] be that one
        uint32_t below = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (((elig >> j) & 1u) && k[j] < prefix && k[j] > below) below = k[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t o = __shfl_xor(below, d, 64);
            below = o > below ? o : below;
        }
        if (l == 0) wmax[w] = below;
        __syncthreads();
        below = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        const float hi = __uint_as_float(prefix);
        floor = (m & 1u) ? hi : 0.5f * ((rank ? hi : __uint_as_float(below)) + hi);
        if (floor == 0.0f || __float_as_uint(floor) == kWfInf) {
            flags |= HD_WF_NO_FLOOR;
            floor = 0.0f;
        } else {
            level = floor * factor[seg < kWaterfallMaxSeg ? seg : kWaterfallMaxSeg];
        }
    }
    // ---- marks: a ballot is bins 1024 w + 64 j .. + 63 = words 32 w + 2 j and 2 j + 1; lane 2 j keeps the low one, lane 2 j + 1 the high one, and the
    // wave stores its 32 words with one 128-byte store.  A flagged row stores zeros.
    uint32_t word = 0, cnt = 0;
    if (flags == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned long long b = __ballot(((elig >> j) & 1u) && __uint_as_float(k[j]) >= level);
            cnt += (uint32_t)__popcll(b);
            if (l == 2u * j) word = (uint32_t)b;
            if (l == 2u * j + 1u) word = (uint32_t)(b >> 32);
        }
    }
    if (l < 32u) rec->marks[32u * w + l] = word;
    if (l == 0) wsum[w] = cnt;
    __syncthreads();
    if (t == 0) {
        rec->flags = flags;
        rec->floor = floor;
        rec->level = level;
        rec->n_marked = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

// One thread per bin and slice of kWfHitRows rows: eight records' flag and mark words in flight, the bits added in registers, one integer atomic per
// thread that counted something (integer sums do not depend on their order: the same pushes give the same bytes).  The flag word of a row is the same
// address for every thread, a mark word for 32 of them.
constexpr uint32_t kWfHitRows = 64;

__global__ __launch_bounds__(256) void k_waterfall_hits(const WaterfallRec* __restrict__ rec, const uint32_t n_rows, uint32_t* __restrict__ hits)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;            // gridDim.x * 256 is exactly kWaterfallBins
    const uint32_t r0 = blockIdx.y * kWfHitRows;
    const uint32_t r1 = r0 + kWfHitRows < n_rows ? r0 + kWfHitRows : n_rows;
    uint32_t h = 0, r = r0;
    for (; r + 8 <= r1; r += 8) {
        uint32_t f[8], m[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { f[u] = rec[r + u].flags; m[u] = rec[r + u].marks[i >> 5]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) h += f[u] == 0 ? (m[u] >> (i & 31u)) & 1u : 0u;
    }
    for (; r < r1; ++r) h += rec[r].flags == 0 ? (rec[r].marks[i >> 5] >> (i & 31u)) & 1u : 0u;
    if (h) atomicAdd(&hits[i], h);
}

void launch_waterfall_detect(hipStream_t st, uint32_t n_rows, const float* rows, const uint32_t* segments, uint32_t seg_full, uint32_t seg_last,
                             uint32_t guard_lo, uint32_t guard_hi, const float* factor, WaterfallRec* out)
{
    hipLaunchKernelGGL(k_waterfall_detect, dim3(n_rows), dim3(kWfThreads), 0, st, rows, segments, seg_full, seg_last, guard_lo, guard_hi, factor, out);
}

void launch_waterfall_hits(hipStream_t st, const WaterfallRec* rec, uint32_t n_rows, uint32_t* hits)
{
    hipLaunchKernelGGL(k_waterfall_hits, dim3(kWaterfallBins / 256, (n_rows + kWfHitRows - 1) / kWfHitRows), dim3(256), 0, st, rec, n_rows, hits);
}

}  // namespace hd
