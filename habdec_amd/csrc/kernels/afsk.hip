// AFSK / AX.25 (hd_afsk_*, include/habdec_amd.h has the definition; host/afsk.hpp restates the kernels).  Not in the reference.
//
// k_afsk_slots: k_fsk4_slots for a real row and two tones.  One workgroup of 256 threads per stream, one launch per chunk of at most HD_AFSK_CHUNK
// samples.  The chunk goes through in tiles of 256 samples, one per thread: a thread quantises its sample and turns it against mark and space, a
// workgroup scan makes the four running sums, which stay in LDS for the whole chunk.  Then a thread per slot that ends in the chunk reads the sums at
// the slot's last sample and W samples earlier -- from LDS inside the chunk, from the stream's rings in device memory when older -- and stores
// d = A_mark - A_space as the slot's record.  The chunk: four running sums of cap + 1 uint32 are 16 (cap + 1) bytes; with the cosine table and the
// waves' totals a chunk of 4096 samples takes 16 * 4100 + 4096 + 64 = 69760 bytes of LDS, two workgroups a CU.
//
// k_afsk_gate: one workgroup per stream over the scan's slots in tiles of 256.  A thread reads its slot's nine levels, a ballot and the waves' counts
// through LDS give every flag its place in the stream's list: slot order, no atomics, whatever the geometry.
//
// k_afsk_frames: one wave per candidate, four candidates per workgroup, nothing shared between them.  The wave loads its phase's levels 64 at a time,
// bit-packed by ballot into LDS, and follows the hard walk's framing on the ballots until it ends; the confidences stay in the slot ring (L2), where
// the metric and the least confident list read them with wave reductions.  Then lane j walks flip pattern j -- lane 0 the untouched one -- with its
// own unstuffing state, CRC and address check (afsk_walk, host/afsk_state.hpp), the lowest counting lane wins by ballot, and that lane walks once more
// to lay the frame's bytes into LDS, from where the wave stores the record.  Integer arithmetic, plain vector stores.
#include <hip/hip_runtime.h>

#include "afsk.h"
#include "wave_util.h"

namespace hd {

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kFrameWaves = 4;
constexpr uint32_t kSlotMask = HD_AFSK_RING - 1u;
constexpr uint32_t kLvBlocks = (afsk_walk_bits(kAfskMaxFrame) + 1u + 63u) / 64u;      // 50: the levels of bit 0 .. L, 64 a block
constexpr uint32_t kDataWords = kAfskMaxFrame / 4u;
static_assert(kAfskMaxFrame % 4u == 0 && sizeof(hd_afsk_candidate) == 48u + kAfskMaxFrame + 4u, "the candidate record: 12 words, the data, a pad word");
static_assert((HD_AFSK_RING & kSlotMask) == 0, "the slot ring is a power of two");

// LDS of a slot launch whose longest row has `cap` samples: P[4][cap1] uint32 | C[1024] | the waves' totals; every part a multiple of 16 bytes
__host__ __device__ __forceinline__ uint32_t lds_cap1(uint32_t cap) { return (cap + 1u + 3u) & ~3u; }
__host__ __device__ __forceinline__ uint32_t lds_bytes(uint32_t cap) { return lds_cap1(cap) * 16u + 1024u * 4u + 4u * kWaves * 4u; }

// (the clocked decoder's range and scale, restated: clocked.hip's is held to its own copy byte for byte)
__device__ __forceinline__ int32_t quantise(float v)
{
    if (v != v) return 0;
    return (int32_t)(fminf(fmaxf(v, -4.0f), 4.0f) * 1024.0f);
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
__device__ __forceinline__ uint64_t lane_get(uint64_t v, uint32_t l) { return ((uint64_t)lane_get((uint32_t)(v >> 32), l) << 32) | lane_get((uint32_t)v, l); }
__device__ __forceinline__ uint64_t lane_xor(uint64_t v, uint32_t o)
{
    return ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)o, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, (int)o, 64);
}
__device__ __forceinline__ uint32_t magnitude(int32_t d) { return d < 0 ? 0u - (uint32_t)d : (uint32_t)d; }

}  // namespace

__global__ __launch_bounds__(256) void k_afsk_slots(const ClockedSrc* __restrict__ src, AfskState* __restrict__ state, uint32_t* ring32_all, size_t ring32_stride,
                                                    const int32_t* __restrict__ ctab, int32_t* slots_all, size_t slot_stride, uint32_t cap)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    AfskState* st = state + s;
    const uint32_t F = uni32(st->F);
    const ClockedSrc d = src[s];
    const uint32_t m = min(uni32(d.n), cap);
    if (!F || !m) return;                                            // no modem, or nothing of this stream in this launch (the whole workgroup)
    const uint32_t cap1 = lds_cap1(cap);
    uint32_t* P = reinterpret_cast<uint32_t*>(smem);                                  // P[k * cap1 + j]: tot[k] after n + j samples
    int32_t* C = reinterpret_cast<int32_t*>(smem + (size_t)cap1 * 16u);
    uint32_t* part32 = reinterpret_cast<uint32_t*>(C + 1024);                         // [4][kWaves]

    const uint32_t W = uni32(st->W);
    const uint32_t phi[2] = {uni32(st->phi[0]), uni32(st->phi[1])};
    const uint64_t n = uni64(st->n), g0 = uni64(st->g);
    uint32_t carry[4];
    for (uint32_t k = 0; k < 4u; ++k) carry[k] = uni32(st->tot[k]);
    const uint32_t* ring32 = ring32_all + (size_t)s * 4u * ring32_stride + kAfskGuard;           // ring k: + k * ring32_stride
    uint32_t first = uni32(d.off);
    if (d.ring_mask) first = uni32(d.sym->base + d.sym->held - d.n_total + d.off);   // the symbol ring's append position is base + held: the call's output ends there

    for (uint32_t a = t; a < 1024u; a += kThreads) C[a] = ctab[a];
    if (t == 0)
        for (uint32_t k = 0; k < 4u; ++k) P[k * cap1] = carry[k];
    __syncthreads();

    // ---- quantise, turn, running sums, tile by tile
    for (uint32_t base = 0; base < m; base += kThreads) {
        const uint32_t j = base + t;
        const bool live = j < m;
        int32_t q = 0;
        if (live) q = quantise(d.ring_mask ? d.p[(first + j) & d.ring_mask] : d.p[first + j]);
        const uint32_t i32 = (uint32_t)n + j;                        // the angle needs i mod 2^32 only
        uint32_t sum[4];
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k) {
            const uint32_t a = (i32 * phi[k]) >> 22;
            sum[2 * k] = (uint32_t)((q * C[a]) >> 15);
            sum[2 * k + 1] = (uint32_t)((-q * C[(a + 768u) & 1023u]) >> 15);
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            sum[k] = wave_scan(sum[k], lane);
            if (lane == 63u) part32[k * kWaves + wave] = sum[k];
        }
        __syncthreads();
#pragma unroll
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
    }

    // ---- the slots whose last sample lies in the chunk: g0 .. g1 - 1, a thread each
    const uint64_t g1 = afsk_slots_before(F, n + m);
    int32_t* slots = slots_all + (size_t)s * slot_stride + kAfskGuard;
    for (uint64_t g = g0 + t; g < g1; g += kThreads) {
        const uint64_t end = afsk_slot_end(F, g);
        const uint32_t j = (uint32_t)(end - n);                      // n <= end < n + m by the choice of g0 and g1 ...
        if (end < n || j >= m) continue;                             // ... (and a state that says otherwise writes nothing)
        const bool from_lds = j + 1u >= W, none = end + 1u <= W;     // the lagged index lies in the chunk / in front of index 0
        uint32_t A[2];
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k) {
            int32_t w[2];
#pragma unroll
            for (uint32_t c = 0; c < 2u; ++c) {
                const uint32_t r = 2u * k + c;
                uint32_t lag = 0;
                if (from_lds) lag = P[r * cap1 + j + 1u - W];
                else if (!none) lag = ring32[r * ring32_stride + ((uint32_t)(end + 1u - W) & (kAfskRing32 - 1u))];
                w[c] = (int32_t)(P[r * cap1 + j + 1u] - lag);
            }
            A[k] = isqrt((uint64_t)((int64_t)w[0] * w[0] + (int64_t)w[1] * w[1]));
        }
        slots[(uint32_t)g & kSlotMask] = (int32_t)A[0] - (int32_t)A[1];
    }
    __syncthreads();                                                 // every lagged value has been read: the chunk's newest sums go over the oldest
    {
        uint32_t* r32 = ring32_all + (size_t)s * 4u * ring32_stride + kAfskGuard;
        for (uint32_t j = (m > kAfskRing32 ? m - kAfskRing32 : 0u) + t; j < m; j += kThreads)
            for (uint32_t k = 0; k < 4u; ++k) r32[k * ring32_stride + ((uint32_t)(n + j + 1u) & (kAfskRing32 - 1u))] = P[k * cap1 + j + 1u];
    }
    if (t == 0) {
        st->n = n + m; st->g = g1 > g0 ? g1 : g0;
        for (uint32_t k = 0; k < 4u; ++k) st->tot[k] = carry[k];
    }
}

__global__ __launch_bounds__(256) void k_afsk_gate(const AfskGate* __restrict__ gate, const int32_t* __restrict__ slots_all, size_t slot_stride, uint32_t* count_all,
                                                   uint32_t* list_all, size_t list_stride, uint32_t list_cap)
{
    __shared__ uint32_t part[kWaves];
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t n = uni32(gate[s].n);
    const uint64_t base = uni64(gate[s].base);
    const int32_t* ring = slots_all + (size_t)s * slot_stride + kAfskGuard;
    uint32_t* list = list_all + (size_t)s * list_stride + kAfskGuard;
    uint32_t running = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += kThreads) {                  // (n is the workgroup's: every thread takes every barrier)
        const uint32_t i = b0 + t;
        const uint64_t g = base + i;
        bool flag = false;
        if (i < n && g >= kAfskBack) {
            // the levels of bit k - 8 .. k: a change, six bits without one, a change
            uint32_t lv = 0;
#pragma unroll
            for (uint32_t j = 0; j < 9u; ++j) lv |= (uint32_t)(ring[(uint32_t)(g - 8u * (8u - j)) & kSlotMask] > 0) << j;
            flag = lv == 0x0FEu || lv == 0x101u;                     // l0 != l1 = ... = l7 != l8
        }
        const uint64_t bal = __ballot(flag);
        if (lane == 0) part[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = running, all = running;
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint32_t p = part[w];
            if (w < wave) before += p;
            all += p;
        }
        if (flag) {
            const uint32_t at = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            if (at < list_cap) list[at] = i;
        }
        running = all;
        __syncthreads();
    }
    if (t == 0) count_all[kAfskGuard + s] = min(running, list_cap);
}

__global__ __launch_bounds__(kFrameWaves * 64) void k_afsk_frames(const AfskCand* __restrict__ cand, const AfskPatterns* __restrict__ pat, uint32_t require_addr,
                                                                  const int32_t* __restrict__ slots_all, size_t slot_stride, const uint32_t* __restrict__ list_all,
                                                                  size_t list_stride, hd_afsk_candidate* __restrict__ out, uint32_t out_cap)
{
    __shared__ uint32_t lds_lv[kFrameWaves][2 * kLvBlocks];          // the levels of bit 0 .. L, bit r of the phase at bit r & 31 of word r >> 5
    __shared__ uint32_t lds_list[kFrameWaves][64];                   // the least confident bits
    __shared__ uint32_t lds_data[kFrameWaves][kDataWords];           // the frame's bytes
    const uint32_t lane = threadIdx.x & 63u, wave = uni32(threadIdx.x >> 6);
    const uint32_t s = blockIdx.y;
    const uint32_t idx = blockIdx.x * kFrameWaves + wave;
    if (idx >= uni32(cand[s].n)) return;                             // (a whole wave leaves: nothing below waits for another wave)
    const uint32_t where = uni32(cand[s].out_off) + idx;
    if (where >= out_cap) return;                                    // (cannot be: a launch has at most out_cap candidates)
    const uint64_t slot = uni64(cand[s].base) + uni32(list_all[(size_t)s * list_stride + kAfskGuard + uni32(cand[s].off) + idx]);
    const int32_t* ring = slots_all + (size_t)s * slot_stride + kAfskGuard;
    const uint32_t L = min(uni32(pat->L), 64u * kLvBlocks - 1u), max_bytes = min(uni32(pat->max_frame_bytes), kAfskMaxFrame);
    const uint32_t n_pat = min(uni32(pat->count), kAfskMaxPatterns), want = min(uni32(pat->list), 63u);
    uint32_t* lv = lds_lv[wave];
    uint32_t* list = lds_list[wave];
    uint32_t* data = lds_data[wave];

    // ---- the levels, 64 at a time, and the framing of the hard walk on the ballots
    uint32_t kind = kAfskOpen, at = L, ones = 0, kept = 0, prev = 0;
    bool done = false;
    for (uint32_t blk = 0; !done && 64u * blk <= L; ++blk) {
        const uint32_t r0 = 64u * blk + lane;
        const uint64_t bal = __ballot(r0 <= L && ring[(uint32_t)(slot + 8u * (uint64_t)r0) & kSlotMask] > 0);
        if (lane == 0) { lv[2u * blk] = (uint32_t)bal; lv[2u * blk + 1u] = (uint32_t)(bal >> 32); }
        const uint32_t top = min(64u, L + 1u - 64u * blk);
        for (uint32_t b = 0; b < top; ++b) {
            const uint32_t level = (uint32_t)(bal >> b) & 1u, r = 64u * blk + b;
            if (!r) { prev = level; continue; }
            const bool one = level == prev;
            prev = level;
            if (one) {
                if (++ones == 7u) { kind = kAfskAbort; at = r; done = true; break; }
                ++kept;
            } else {
                const uint32_t was = ones;
                ones = 0;
                if (was == 5u) continue;
                if (was == 6u) { kind = kAfskClose; at = r; done = true; break; }
                ++kept;
            }
        }
    }                                                                // (not done: open, at the walk's last bit L)
    kind = uni32(kind); at = uni32(at); kept = uni32(kept);
    const uint32_t fed = kept >= 7u ? kept - 7u : 0u;
    const bool shaped = kind == kAfskClose && !(fed & 7u) && (fed >> 3) >= kAfskMinFrame && (fed >> 3) <= max_bytes;

    // ---- the metric: |d| over the walked bits
    uint64_t msum = 0;
    for (uint32_t r = 1u + lane; r <= at; r += 64u) msum += magnitude(ring[(uint32_t)(slot + 8u * (uint64_t)r) & kSlotMask]);
    const uint64_t metric = lane_get(wave_scan(msum, lane), 63u);

    uint32_t result = kind == kAfskAbort ? HD_AFSK_ABORT : kind == kAfskOpen ? HD_AFSK_OPEN : HD_AFSK_UNSHAPED;
    uint32_t len = 0, flips = 0, addr_ok = 0, fcs = 0;
    for (uint32_t k = lane; k < kDataWords; k += 64u) data[k] = 0u;
    wave_lds_sync();

    if (shaped) {
        // ---- the least confident levels of the bits 1 .. at - 8: keys (confidence, bit) in increasing order, one wave minimum a round
        uint32_t nl = 0;
        uint64_t last = 0;
        for (; nl < want && n_pat > 1u; ++nl) {
            uint64_t best = ~0ull;
            for (uint32_t r = 1u + lane; r + 8u <= at; r += 64u) {
                const uint64_t key = ((uint64_t)magnitude(ring[(uint32_t)(slot + 8u * (uint64_t)r) & kSlotMask]) << 12) | r;
                if ((!nl || key > last) && key < best) best = key;
            }
            for (uint32_t o = 1; o < 64u; o <<= 1) {
                const uint64_t other = lane_xor(best, o);
                best = other < best ? other : best;
            }
            if (best == ~0ull) break;
            if (lane == 0) list[nl] = (uint32_t)best & 0xFFFu;
            last = best;
        }
        wave_lds_sync();

        // ---- lane j walks pattern j
        uint64_t m = lane < n_pat ? pat->mask[lane] : 0ull;
        const uint32_t my_flips = (uint32_t)__popcll(m);
        bool fits = lane < n_pat;
        auto next_flip = [&]() {                                     // the bit the mask's lowest position stands for; ~0: none (it equals no bit)
            if (!m) return ~0u;
            const uint32_t pos = (uint32_t)__builtin_ctzll(m);
            m &= m - 1ull;
            if (pos >= nl) { fits = false; return ~0u; }
            return list[pos];
        };
        static_assert(kAfskMaxFlips == 4u, "four flips, a register each");
        const uint32_t f0 = next_flip(), f1 = next_flip(), f2 = next_flip(), f3 = next_flip();
        if (m) fits = false;
        auto level = [=](uint32_t r) { return ((lv[r >> 5] >> (r & 31u)) & 1u) ^ (uint32_t)(r == f0 || r == f1 || r == f2 || r == f3); };
        AfskWalk w{kAfskOpen, 0u, 0u, 0u, 0u, 0u, 0u};
        if (fits) w = afsk_walk(level, at, max_bytes, [](uint32_t, uint32_t) {});
        const bool framed = fits && w.kind == kAfskClose && w.at == at && w.shaped && w.fcs_ok;
        const uint64_t counting = __ballot(framed && w.addr_ok), turned_away = __ballot(framed && !w.addr_ok);
        uint32_t winner = 0;
        if (counting & 1ull) result = HD_AFSK_PLAIN;
        else if (turned_away & 1ull) result = require_addr ? HD_AFSK_REFUSED : HD_AFSK_PLAIN;
        else if (counting) { result = HD_AFSK_REPAIRED; winner = (uint32_t)__builtin_ctzll(counting); }
        else result = turned_away ? HD_AFSK_REFUSED : HD_AFSK_FCS_FAILED;

        // ---- the winner's bytes (the hard walk's where none won)
        if (lane == winner) {
            uint8_t* bytes = reinterpret_cast<uint8_t*>(data);
            w = afsk_walk(level, at, max_bytes, [&](uint32_t i, uint32_t b) { if (i < kAfskMaxFrame) bytes[i] = (uint8_t)b; });
        }
        len = lane_get(w.bits, winner) >> 3; addr_ok = lane_get(w.addr_ok, winner); fcs = lane_get(w.fcs, winner);
        flips = lane_get(my_flips, winner);
        wave_lds_sync();
    }

    hd_afsk_candidate* o = out + where;
    if (lane == 0) {
        o->slot = slot; o->close_slot = kind == kAfskClose ? slot + 8u * (uint64_t)at : 0ull; o->metric = metric;
        o->result = result; o->bits = at; o->len = len; o->flips = flips; o->addr_ok = addr_ok; o->fcs = fcs;
        o->_pad = 0u;
    }
    uint32_t* words = reinterpret_cast<uint32_t*>(o->data);
    for (uint32_t k = lane; k < kDataWords; k += 64u) words[k] = data[k];
}

uint32_t afsk_slots_lds_bytes(uint32_t cap) { return cap && cap <= HD_AFSK_CHUNK && lds_bytes(cap) <= 160u * 1024u ? lds_bytes(cap) : 0u; }

bool launch_afsk_slots(hipStream_t st, uint32_t n_streams, uint32_t cap, const ClockedSrc* src, AfskState* state, uint32_t* ring32, size_t ring32_stride,
                       const int32_t* ctab, int32_t* slots, size_t slot_stride)
{
    const uint32_t bytes = afsk_slots_lds_bytes(cap);
    if (!bytes) return false;
    if (bytes > 64u * 1024u && hipFuncSetAttribute(reinterpret_cast<const void*>(k_afsk_slots), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return false;
    hipLaunchKernelGGL(k_afsk_slots, dim3(n_streams), dim3(kThreads), bytes, st, src, state, ring32, ring32_stride, ctab, slots, slot_stride, cap);
    return true;
}

void launch_afsk_gate(hipStream_t st, uint32_t n_streams, const AfskGate* gate, const int32_t* slots, size_t slot_stride, uint32_t* count, uint32_t* list,
                      size_t list_stride, uint32_t list_cap)
{
    if (!n_streams) return;
    hipLaunchKernelGGL(k_afsk_gate, dim3(n_streams), dim3(kThreads), 0, st, gate, slots, slot_stride, count, list, list_stride, list_cap);
}

void launch_afsk_frames(hipStream_t st, uint32_t n_streams, uint32_t cap, const AfskCand* cand, const AfskPatterns* pat, uint32_t require_addr,
                        const int32_t* slots, size_t slot_stride, const uint32_t* list, size_t list_stride, hd_afsk_candidate* out, uint32_t out_cap)
{
    if (!cap || !n_streams) return;
    hipLaunchKernelGGL(k_afsk_frames, dim3((cap + kFrameWaves - 1u) / kFrameWaves, n_streams), dim3(kFrameWaves * 64u), 0, st, cand, pat, require_addr, slots,
                       slot_stride, list, list_stride, out, out_cap);
}

}  // namespace hd
