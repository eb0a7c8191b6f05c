// Clocked soft-decision character decoder (hd_clocked_*, include/habdec_amd.h has the definition; host/clocked.hpp restates it position by position).
// Not in the reference.
//
// k_clocked: one wave per stream.  A stream's sample history is kept as running sums: word (i & (RING - 1)) of its ring is P_i = q_0 + ... + q_{i-1} mod
// 2^32 for the newest RING indices i <= n, so every S(a, b) of the definition is P_b - P_a, one subtraction (|S| < 2^31: exact).  The push is quantised
// 64 samples at a time, a wave scan makes their running sums.  What the cursor can reach in this launch -- P_{p-h} .. P_n, at most look + h + the
// push -- is then copied into LDS once, and the walk reads LDS only: 64 positions take the edge test at once and a ballot finds the edges of the block;
// the refinement is a wave-wide minimum over (cost, index) packed into one 64-bit key, the lowest index winning; lane k loads boundary k, a neighbour
// exchange gives the bit sums, a second ballot the character.  Integer arithmetic behind the quantisation, no atomics.
//
// One arithmetic, like baud_probe.hip: not compiled per mode.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "wave_util.h"

namespace hd {

namespace {

constexpr uint32_t kRingMask = HD_CLOCKED_RING - 1u;

// (Not to be merged with tones.hip's quantise, another range and scale: each is held to its host restatement -- clocked_quantise, tones_quantise --
// precisely because kernel and restatement are written separately.)
__device__ __forceinline__ int32_t quantise(float v, uint32_t invert)
{
    if (v != v) return 0;
    const int32_t q = (int32_t)(fminf(fmaxf(v, -4.0f), 4.0f) * 1024.0f);
    return invert ? -q : q;
}

// the launch's window of running sums in LDS: P_i at word i - lo (the index is clamped: nothing outside the window is ever asked for)
struct Window {
    const uint32_t* w;
    uint64_t lo;
    uint32_t words;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return w[min((uint32_t)(i - lo), words - 1u)]; }
};

}  // namespace

__global__ __launch_bounds__(64) void k_clocked(const ClockedSrc* __restrict__ src, ClockedState* __restrict__ state, uint32_t* ring_all, size_t ring_stride,
                                                uint32_t* rec_all, size_t rec_stride, uint32_t record_cap, uint32_t lds_words)
{
    extern __shared__ uint32_t win[];
    const uint32_t s = blockIdx.x, l = threadIdx.x;
    ClockedState* st = state + s;
    const uint32_t F = uni32(st->F);
    if (!F) return;                                                  // the stream is off
    const ClockedSrc d = src[s];
    const uint32_t m = uni32(d.n) <= HD_CLOCKED_CHUNK ? uni32(d.n) : HD_CLOCKED_CHUNK;
    uint32_t* ring = ring_all + (size_t)s * ring_stride + kClockedGuard;
    uint32_t* rec = rec_all + (size_t)s * rec_stride + kClockedGuard;
    const uint32_t nbits = uni32(st->nbits), nstops = uni32(st->nstops), invert = uni32(st->invert);
    uint64_t n = uni64(st->n), p = uni64(st->p);

    // ---- append: P_{n+1} .. P_{n+m}
    if (m) {
        uint32_t total = uni32(st->total);
        uint32_t first = d.off;
        if (d.ring_mask) first = d.sym->base + d.sym->held - d.n_total + d.off;      // the ring's append position is base + held: the call's output ends there
        for (uint32_t b = 0; b < m; b += 64u) {
            const uint32_t j = b + l;
            int32_t q = 0;
            if (j < m) q = quantise(d.ring_mask ? d.p[(first + j) & d.ring_mask] : d.p[first + j], invert);
            uint32_t sum = (uint32_t)q;                              // inclusive scan over the wave (wave_util.h's wave_scan, written out: see there)
            for (uint32_t o = 1; o < 64u; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)sum, o, 64);
                if (l >= o) sum += up;
            }
            sum += total;
            if (j < m) ring[(uint32_t)(n + j + 1u) & kRingMask] = sum;
            total = (uint32_t)__builtin_amdgcn_readlane((int)sum, 63);
        }
        n += m;
        if (l == 0) { st->total = total; st->n = n; }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");           // the lanes read each other's sums back from memory
    }

    // ---- scan
    const uint32_t full = (F + 32768u) >> 16, h = max(2u, (F + 65536u) >> 17), K = 1u + nbits + nstops;
    const uint32_t look = h + (uint32_t)(((uint64_t)K * F + 32768u) >> 16);
    const uint32_t skip = (uint32_t)(((uint64_t)(2u * (1u + nbits) + 1u) * F + 65536u) >> 17);
    if (p + look > n) return;                                        // nothing can be decided yet (the whole wave)
    // the window: the cursor only moves forward, and no decision reads behind p - h or beyond n (n - p < look + the push: the host sized the LDS)
    Window at;
    at.w = win; at.lo = p - h; at.words = lds_words;
    {
        const uint32_t count = min((uint32_t)(n - at.lo) + 1u, lds_words);
        for (uint32_t i = l; i < count; i += 64u) win[i] = ring[(uint32_t)(at.lo + i) & kRingMask];
        __syncthreads();                                             // (one wave)
    }
    uint64_t chars = uni64(st->chars), rejects = uni64(st->rejects), dropped = uni64(st->dropped), written = uni64(st->written), taken = uni64(st->taken);
    while (p + look <= n) {
        const uint64_t last = n - look, base = p;                    // the last position that can be decided; the block of 64 positions from p on
        const uint32_t valid = last - p >= 63u ? 64u : (uint32_t)(last - p) + 1u;
        bool e = false;
        if (l < valid) {
            const uint64_t x = p + l;
            const uint32_t a = at(x - h), b = at(x), c = at(x + h);
            e = (int32_t)(b - a) > 0 && (int32_t)(c - b) < 0;
        }
        uint64_t edges = __ballot(e);
        p = base + valid;                                            // where the cursor stands when every edge of the block is rejected
        while (edges) {
            const uint64_t cand = base + (uint32_t)__builtin_ctzll(edges);
            edges &= edges - 1ull;
            // the start edge: the smallest x in [cand, cand + h] that minimises S(x, x + full) - S(x - h, x)
            unsigned long long key = ~0ull;
            for (uint32_t i = l; i <= h; i += 64u) {
                const uint64_t x = cand + i;
                const uint32_t a = at(x - h), b = at(x), c = at(x + full);
                const int32_t cost = (int32_t)(c - b) - (int32_t)(b - a);
                const unsigned long long k = ((unsigned long long)((uint32_t)cost ^ 0x80000000u) << 32) | i;
                key = k < key ? k : key;
            }
            for (uint32_t o = 32; o; o >>= 1) {
                const unsigned long long other = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), o, 64) << 32) |
                                                 (uint32_t)__shfl_xor((int)(uint32_t)key, o, 64);
                key = other < key ? other : key;
            }
            const uint64_t x = cand + uni32((uint32_t)key);
            // bit sums: lane k holds P at boundary k
            uint32_t pb = 0;
            if (l <= K) pb = at(x + (uint32_t)(((uint64_t)l * F + 32768u) >> 16));
            const int32_t bit = (int32_t)((uint32_t)__shfl_down((int)pb, 1, 64) - pb);      // lane k < K: the sum over bit k of the character
            const int32_t start = __builtin_amdgcn_readlane(bit, 0), stop = __builtin_amdgcn_readlane(bit, 1 + (int)nbits);
            if (!(start < 0 && stop > 0)) { rejects += 1; continue; }                       // (p += 1: the block's next edge, if it has one)
            const uint32_t ch = (uint32_t)(__ballot(l >= 1u && l <= nbits && bit > 0) >> 1);
            if (written - taken >= record_cap) { taken += 1; dropped += 1; }
            uint32_t* r = rec + (size_t)(written % record_cap) * kClockedRecWords;
            // words of hd_clocked_record: pos, data[8], start, stop, stop2, ch
            const int32_t data = __shfl_up(bit, 1, 64);              // lane 2 + k takes data_k from lane 1 + k
            const int32_t stop2 = __builtin_amdgcn_readlane(bit, 2 + (int)nbits);
            uint32_t w = 0;
            if (l == 0) w = (uint32_t)x;
            else if (l == 1) w = (uint32_t)(x >> 32);
            else if (l < 10u) w = l - 2u < nbits ? (uint32_t)data : 0u;
            else if (l == 10u) w = (uint32_t)start;
            else if (l == 11u) w = (uint32_t)stop;
            else if (l == 12u) w = nstops == 2u ? (uint32_t)stop2 : 0u;
            else w = ch;
            if (l < kClockedRecWords) r[l] = w;
            written += 1; chars += 1;
            p = x + skip;
            break;
        }
    }
    if (l == 0) {
        st->p = p; st->chars = chars; st->rejects = rejects; st->dropped = dropped; st->written = written; st->taken = taken;
    }
}

bool launch_clocked(hipStream_t st, uint32_t n_streams, const ClockedSrc* src, ClockedState* state, uint32_t* ring, size_t ring_stride, uint32_t* rec,
                    size_t rec_stride, uint32_t record_cap, uint32_t lds_words)
{
    const uint32_t bytes = lds_words * (uint32_t)sizeof(uint32_t);
    if (bytes > 160u * 1024u) return false;
    if (bytes > 64u * 1024u && hipFuncSetAttribute(reinterpret_cast<const void*>(k_clocked), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return false;
    hipLaunchKernelGGL(k_clocked, dim3(n_streams), dim3(64), bytes, st, src, state, ring, ring_stride, rec, rec_stride, record_cap, lds_words);
    return true;
}

}  // namespace hd
