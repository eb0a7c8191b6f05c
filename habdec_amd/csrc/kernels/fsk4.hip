// Horus Binary 4FSK (hd_fsk4_*, include/habdec_amd.h has the definition; host/fsk4.hpp restates both kernels).  Not in the reference.
//
// k_fsk4_slots: one workgroup of 256 threads per stream, one launch per chunk of at most HD_FSK4_CHUNK samples, laid out like k_tones.  The chunk goes
// through in tiles of 256 samples, one per thread: a thread quantises its sample and turns it against the four tones, a workgroup scan (wave scan, then
// the waves' totals through LDS) makes the eight running sums, which stay in LDS for the whole chunk.  Only then the envelopes are taken, and only where
// the timing grid has a slot: a thread per slot that ends in the chunk reads the sums at the slot's last sample and W samples earlier -- from LDS
// inside the chunk, from the stream's rings in device memory when older -- and stores the four envelopes as one 16-byte record.  At 8 samples per
// symbol every sample ends a slot, at 2048 every 256th.  The rings are only read until the last slot is done, then the chunk's newest sums are stored
// over the oldest.  Integer arithmetic behind the quantisation, no atomics, plain vector stores.
//
// The chunk: eight running sums of cap + 1 uint32 each are 32 (cap + 1) bytes; with the cosine table (4096 bytes) and the waves' totals (128 bytes) a
// chunk of 4096 samples takes 32 * 4100 + 4096 + 128 = 135424 of gfx950's 163840 bytes of LDS.  The next power of two does not fit, and a chunk that
// is none would cut pushes of 4096 -- the commonest -- in two; one workgroup per CU is what a stream per workgroup asks for anyway.
//
// k_fsk4_frames: one wave per candidate, four candidates per workgroup, nothing shared between them (a wave that fails the unique-word gate leaves at
// once, so only wave-wide synchronisation is used).  Steps 1 .. 6 of the definition; the K 2^chase_bits flip patterns are spread over the lanes with a
// codeword's patterns in neighbouring lanes, so the cheapest pattern is a butterfly minimum over 2^chase_bits lanes.
#include <hip/hip_runtime.h>

#include "fsk4.h"
#include "wave_util.h"

namespace hd {

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kFrameWaves = 4;

// LDS of a slot launch whose longest row has `cap` samples: P[8][cap1] uint32 | C[1024] | the waves' totals; every part a multiple of 16 bytes
__host__ __device__ __forceinline__ uint32_t lds_cap1(uint32_t cap) { return (cap + 1u + 3u) & ~3u; }
__host__ __device__ __forceinline__ uint32_t lds_bytes(uint32_t cap) { return lds_cap1(cap) * 32u + 1024u * 4u + 8u * kWaves * 4u; }

// (the tones object's range and scale, restated: tones.hip's rows are held to its own copy byte for byte)
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

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lane_get(uint32_t v, uint32_t l) { return (uint32_t)__shfl((int)v, (int)l, 64); }
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, uint32_t o) { return (uint32_t)__shfl_xor((int)v, (int)o, 64); }

}  // namespace

__global__ __launch_bounds__(256) void k_fsk4_slots(const TonesSrc* __restrict__ src, Fsk4State* __restrict__ state, uint32_t* ring32_all, size_t ring32_stride,
                                                    const int32_t* __restrict__ ctab, uint32_t* slots_all, size_t slot_stride, uint32_t slot_mask, uint32_t cap)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    Fsk4State* st = state + s;
    const uint32_t F = uni32(st->F);
    const TonesSrc d = src[s];
    const uint32_t m = min(uni32(d.n), cap), off = uni32(d.off);
    if (!F || !m) return;                                            // no modem, or nothing of this stream in this launch (the whole workgroup)
    const uint32_t cap1 = lds_cap1(cap);
    uint32_t* P = reinterpret_cast<uint32_t*>(smem);                                  // P[k * cap1 + j]: tot[k] after n + j samples
    int32_t* C = reinterpret_cast<int32_t*>(smem + (size_t)cap1 * 32u);
    uint32_t* part32 = reinterpret_cast<uint32_t*>(C + 1024);                         // [8][kWaves]

    const uint32_t W = uni32(st->W);
    uint32_t phi[4], psi[4];
    for (uint32_t k = 0; k < 4u; ++k) { phi[k] = uni32(st->phi[k]); psi[k] = uni32(st->psi[k]); }
    const uint64_t n = uni64(st->n), g0 = uni64(st->g);
    uint32_t carry[8];
    for (uint32_t k = 0; k < 8u; ++k) carry[k] = uni32(st->tot[k]);
    const uint32_t* ring32 = ring32_all + (size_t)s * 8u * ring32_stride + kFsk4Guard;           // ring k: + k * ring32_stride

    for (uint32_t a = t; a < 1024u; a += kThreads) C[a] = ctab[a];
    if (t == 0)
        for (uint32_t k = 0; k < 8u; ++k) P[k * cap1] = carry[k];
    __syncthreads();

    // ---- quantise, rotate, running sums, tile by tile
    for (uint32_t base = 0; base < m; base += kThreads) {
        const uint32_t j = base + t;
        const bool live = j < m;
        int32_t q_re = 0, q_im = 0;
        if (live) {
            const float2 v = d.p[off + j];
            q_re = quantise(v.x); q_im = quantise(v.y);
        }
        const uint32_t i32 = (uint32_t)n + j;                        // theta needs i mod 2^32 only
        uint32_t sum[8];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t a = (i32 * phi[k] + psi[k]) >> 22;
            const int32_t c = C[a], sn = C[(a + 768u) & 1023u];
            sum[2 * k] = (uint32_t)((q_re * c + q_im * sn) >> 15);
            sum[2 * k + 1] = (uint32_t)((q_im * c - q_re * sn) >> 15);
        }
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            sum[k] = wave_scan(sum[k], lane);
            if (lane == 63u) part32[k * kWaves + wave] = sum[k];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
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
    }

    // ---- the slots whose last sample lies in the chunk: g0 .. g1 - 1, a thread each
    const uint64_t g1 = fsk4_slots_before(F, n + m);
    uint32_t* slots = slots_all + (size_t)s * slot_stride + kFsk4Guard;
    for (uint64_t g = g0 + t; g < g1; g += kThreads) {
        const uint64_t end = fsk4_slot_end(F, g);
        const uint32_t j = (uint32_t)(end - n);                      // n <= end < n + m by the choice of g0 and g1 ...
        if (end < n || j >= m) continue;                             // ... (and a state that says otherwise writes nothing)
        const bool from_lds = j + 1u >= W, none = end + 1u <= W;     // the lagged index lies in the chunk / in front of index 0
        uint32_t A[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            int32_t w[2];
#pragma unroll
            for (uint32_t c = 0; c < 2u; ++c) {
                const uint32_t r = 2u * k + c;
                uint32_t lag = 0;
                if (from_lds) lag = P[r * cap1 + j + 1u - W];
                else if (!none) lag = ring32[r * ring32_stride + ((uint32_t)(end + 1u - W) & (kFsk4Ring32 - 1u))];
                w[c] = (int32_t)(P[r * cap1 + j + 1u] - lag);
            }
            A[k] = isqrt((uint64_t)((int64_t)w[0] * w[0] + (int64_t)w[1] * w[1]));
        }
        *reinterpret_cast<uint4*>(slots + (size_t)((uint32_t)g & slot_mask) * 4u) = make_uint4(A[0], A[1], A[2], A[3]);
    }
    __syncthreads();                                                 // every lagged value has been read: the chunk's newest sums go over the oldest
    {
        uint32_t* r32 = ring32_all + (size_t)s * 8u * ring32_stride + kFsk4Guard;
        for (uint32_t j = (m > kFsk4Ring32 ? m - kFsk4Ring32 : 0u) + t; j < m; j += kThreads)
            for (uint32_t k = 0; k < 8u; ++k) r32[k * ring32_stride + ((uint32_t)(n + j + 1u) & (kFsk4Ring32 - 1u))] = P[k * cap1 + j + 1u];
    }
    if (t == 0) {
        st->n = n + m; st->g = g1 > g0 ? g1 : g0;
        for (uint32_t k = 0; k < 8u; ++k) st->tot[k] = carry[k];
    }
}

__global__ __launch_bounds__(kFrameWaves * 64) void k_fsk4_frames(const Fsk4Cand* __restrict__ cand, const Fsk4Tab* __restrict__ tabs,
                                                                  const uint32_t* __restrict__ slots_all, size_t slot_stride, uint32_t slot_mask,
                                                                  uint32_t uw_max_errors, uint32_t chase_bits, uint32_t* cnt, Fsk4Out* __restrict__ out,
                                                                  uint32_t out_cap)
{
    __shared__ int32_t lds_soft[kFrameWaves][2 * kFsk4MaxSymbols];                   // a frame's soft bits, on-air order
    __shared__ int32_t lds_cv[kFrameWaves][23 * kFsk4MaxCodewords + 6];              // ... gathered: word k's position b at 23 k + b
    __shared__ uint32_t lds_hw[kFrameWaves][kFsk4MaxCodewords], lds_lc[kFrameWaves][kFsk4MaxCodewords], lds_cw[kFrameWaves][kFsk4MaxCodewords];
    __shared__ uint32_t lds_pay[kFrameWaves][kFsk4MaxPayload];
    const uint32_t lane = threadIdx.x & 63u, wave = uni32(threadIdx.x >> 6);
    const uint32_t s = blockIdx.y;
    const uint32_t idx = blockIdx.x * kFrameWaves + wave;
    if (idx >= uni32(cand[s].n)) return;                             // (a whole wave leaves: nothing below waits for another wave)
    const uint64_t slot = uni64(cand[s].base) + uni32(cand[s].off) + idx;
    const uint4* ring = reinterpret_cast<const uint4*>(slots_all + (size_t)s * slot_stride + kFsk4Guard);
    const Fsk4Tab* tab = tabs + s;
    const uint32_t nsym = min(uni32(tab->nsym), kFsk4MaxSymbols), K = min(uni32(tab->K), kFsk4MaxCodewords), P = min(uni32(tab->P), kFsk4MaxPayload);
    const uint32_t poly = uni32(tab->poly), uw = uni32(tab->uw);
    chase_bits = min(chase_bits, 6u);
    int32_t* soft = lds_soft[wave];
    int32_t* cv = lds_cv[wave];
    uint32_t *hw = lds_hw[wave], *lc = lds_lc[wave], *cwb = lds_cw[wave], *pay = lds_pay[wave];

    // ---- 1, 2: the hard symbols of the unique word, lanes 0 .. 7
    uint32_t wrong = 0;
    if (lane < 8u) {
        const uint4 E = ring[((uint32_t)slot + 8u * lane) & slot_mask];
        uint32_t best = 0, top = E.x;
        if (E.y > top) { best = 1; top = E.y; }
        if (E.z > top) { best = 2; top = E.z; }
        if (E.w > top) { best = 3; }
        wrong = best ^ ((uw >> (14u - 2u * lane)) & 3u);
    }
    const uint32_t uw_err = (uint32_t)__popcll(__ballot(wrong & 1u)) + (uint32_t)__popcll(__ballot(wrong & 2u));
    if (uw_err > uw_max_errors) return;

    // ---- 3: soft bits of every symbol, and the metric
    uint64_t msum = 0;
    for (uint32_t m = lane; m < nsym; m += 64u) {
        const uint4 E = ring[((uint32_t)slot + 8u * m) & slot_mask];
        const uint32_t m01 = max(E.x, E.y), m23 = max(E.z, E.w), m02 = max(E.x, E.z), m13 = max(E.y, E.w);
        soft[2u * m] = (int32_t)m23 - (int32_t)m01;
        soft[2u * m + 1u] = (int32_t)m13 - (int32_t)m02;
        msum += max(m01, m23);
    }
    msum = wave_scan(msum, lane);
    const uint64_t metric = ((uint64_t)lane_get((uint32_t)(msum >> 32), 63u) << 32) | lane_get((uint32_t)msum, 63u);
    wave_lds_sync();

    // ---- 4: descramble, de-interleave, gather
    for (uint32_t e = lane; e < 23u * K; e += 64u) {
        const uint32_t where = tab->src[e];
        int32_t v = -kFsk4PadConfidence;
        if (where != kFsk4SrcPad) {
            v = soft[min(where & 0x3FFu, 2u * kFsk4MaxSymbols - 1u)];
            if (where & 0x8000u) v = -v;
        }
        cv[e] = v;
    }
    wave_lds_sync();

    // ---- 5: per word, lane k: the hard word and its least confident positions (five bits each in lc) ...
    if (lane < K) {
        const int32_t* c = cv + 23u * lane;
        uint32_t h = 0;
        for (uint32_t b = 0; b < 23u; ++b) h |= (uint32_t)(c[b] > 0) << (22u - b);
        uint32_t taken = 0, packed = 0;
        for (uint32_t i = 0; i < chase_bits; ++i) {
            uint32_t pick = 23u, least = 0xFFFFFFFFu;
            for (uint32_t b = 0; b < 23u; ++b) {
                const uint32_t conf = (uint32_t)abs(c[b]);
                if (!((taken >> b) & 1u) && (pick == 23u || conf < least)) { pick = b; least = conf; }
            }
            taken |= 1u << pick; packed |= pick << (5u * i);
        }
        hw[lane] = h; lc[lane] = packed;
    }
    wave_lds_sync();
    // ... then a lane per (word, flip pattern), a word's patterns side by side
    const uint32_t total = K << chase_bits, group = 1u << chase_bits;
    for (uint32_t base = 0; base < total; base += 64u) {
        const uint32_t it = base + lane;
        const bool valid = it < total;
        const uint32_t k = valid ? it >> chase_bits : 0u, pn = it & (group - 1u);
        const uint32_t h = hw[k], packed = lc[k];
        uint32_t w = h;
        for (uint32_t i = 0; i < chase_bits; ++i)
            if ((pn >> i) & 1u) w ^= 1u << (22u - ((packed >> (5u * i)) & 31u));
        const uint32_t cw = w ^ tab->syn[fsk4_rem(w, poly)];
        uint32_t cost = 0;
        for (uint32_t diff = cw ^ h, b = 0; b < 23u; ++b)
            if ((diff >> (22u - b)) & 1u) cost += (uint32_t)abs(cv[23u * k + b]);
        const uint64_t key = valid ? ((uint64_t)cost << 6) | pn : ~0ull;
        uint64_t low = key;
        for (uint32_t o = 1; o < group; o <<= 1) {
            const uint64_t other = ((uint64_t)lane_xor((uint32_t)(low >> 32), o) << 32) | lane_xor((uint32_t)low, o);
            low = other < low ? other : low;
        }
        if (valid && key == low) cwb[k] = cw;                        // (the keys of a word differ in the pattern number: one lane)
    }
    wave_lds_sync();

    // ---- 6: corrected bits, payload, CRC
    uint32_t corr = lane < K ? (uint32_t)__popc(cwb[lane] ^ hw[lane]) : 0u;
    corr = lane_get(wave_scan(corr, lane), 63u);
    if (lane < kFsk4MaxPayload) {
        uint32_t byte = 0;
        if (lane < P)
            for (uint32_t i = 0; i < 8u; ++i) {
                const uint32_t bit = 8u * lane + i;
                byte = byte << 1 | ((cwb[bit / 12u] >> (22u - bit % 12u)) & 1u);
            }
        pay[lane] = byte;
    }
    wave_lds_sync();
    uint32_t at = 0, crc_ok = 0;
    if (lane == 0) {
        uint32_t crc = 0xFFFFu;
        for (uint32_t b = 0; b + 2u < P; ++b) crc = fsk4_crc16_byte(crc, pay[b]);
        crc_ok = P >= 2u && crc == (pay[P - 2u] | pay[P - 1u] << 8);
        at = atomicAdd(cnt, 1u);
    }
    at = uni32(at);
    if (at >= out_cap) return;                                       // (cannot be: a launch has at most out_cap candidates)
    Fsk4Out* o = out + at;
    if (lane == 0) {
        o->slot = slot; o->metric = metric;
        o->stream = s; o->crc_ok = crc_ok; o->corrected = corr; o->uw_errors = uw_err;
    }
    if (lane < kFsk4MaxPayload / 4u)
        reinterpret_cast<uint32_t*>(o->payload)[lane] = pay[4u * lane] | pay[4u * lane + 1u] << 8 | pay[4u * lane + 2u] << 16 | pay[4u * lane + 3u] << 24;
}

bool launch_fsk4_slots(hipStream_t st, uint32_t n_streams, uint32_t cap, const TonesSrc* src, Fsk4State* state, uint32_t* ring32, size_t ring32_stride,
                       const int32_t* ctab, uint32_t* slots, size_t slot_stride, uint32_t slot_cap)
{
    if (!cap || cap > HD_FSK4_CHUNK || !slot_cap || (slot_cap & (slot_cap - 1u))) return false;
    const uint32_t bytes = lds_bytes(cap);
    if (bytes > 160u * 1024u) return false;
    if (bytes > 64u * 1024u && hipFuncSetAttribute(reinterpret_cast<const void*>(k_fsk4_slots), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return false;
    hipLaunchKernelGGL(k_fsk4_slots, dim3(n_streams), dim3(kThreads), bytes, st, src, state, ring32, ring32_stride, ctab, slots, slot_stride, slot_cap - 1u, cap);
    return true;
}

void launch_fsk4_frames(hipStream_t st, uint32_t n_streams, uint32_t cap, const Fsk4Cand* cand, const Fsk4Tab* tab, const uint32_t* slots, size_t slot_stride,
                        uint32_t slot_cap, uint32_t uw_max_errors, uint32_t chase_bits, uint32_t* cnt, Fsk4Out* out, uint32_t out_cap)
{
    if (!cap || !n_streams) return;
    hipLaunchKernelGGL(k_fsk4_frames, dim3((cap + kFrameWaves - 1u) / kFrameWaves, n_streams), dim3(kFrameWaves * 64u), 0, st, cand, tab, slots, slot_stride,
                       slot_cap - 1u, uw_max_errors, chase_bits, cnt, out, out_cap);
}

}  // namespace hd
