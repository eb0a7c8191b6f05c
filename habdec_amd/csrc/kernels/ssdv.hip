// SSDV packets (hd_ssdv_*, include/habdec_amd.h has the definition; host/ssdv.hpp restates the decoder by another route).
//
// k_ssdv_append: the scan round's new words go from the staging buffer into the streams' rings.  k_ssdv_scan: one wave per candidate position.  The wave
// loads the candidate's 256 words (four per lane), keeps the bytes in its own 256 bytes of LDS, and runs the trials of the definition:
//   - syndromes: lane l evaluates root l & 31 over one half of the word by Horner (the half's byte is one LDS address per half: a broadcast), the halves
//     meet through one shuffle;
//   - erasures: the 24 smallest keys by 24 wave minima, once, in front of trial 1 (the three sets nest);
//   - erasure locator and Berlekamp-Massey without an inverse, coefficient c on lane c, the discrepancy by a wave-wide xor;
//   - root search: a lane evaluates the locator at its four positions at once, four field elements packed in a register against a table of powers;
//   - Forney values, the corrected word back into LDS, its syndromes once more (all 32 must vanish: the word IS a codeword then, whatever the path to
//     it), the count of changed bytes outside the erasures against 2 e + f <= 32, and the CRC-32 only then.
// Field products are shift-and-xor, no table in LDS: NOTES.md "SSDV packets" says why.  Plain C++ and vector stores; the only atomics are the integer
// adds that hand out a result slot and sum a stream's crc_bad, so nothing depends on the order in which waves finish (the host sorts the results).
//
// One arithmetic, like clocked.hip and tones.hip: not compiled per mode.
#include <hip/hip_runtime.h>

#include "ssdv.h"
#include "wave_util.h"

namespace hd {

namespace {

constexpr uint32_t kMask = kSsdvRing - 1u;

// LDS written by some lanes of the wave is read by others
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t bit_mask(uint32_t v, uint32_t k) { return 0u - ((v >> k) & 1u); }
// a * alpha modulo 0x187
__device__ __forceinline__ uint32_t xtime(uint32_t a) { return (a << 1) ^ (bit_mask(a, 7) & 0x187u); }
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) { p ^= a & bit_mask(b, k); a = xtime(a); }
    return p;
}
// four field elements packed in v, each times b
__device__ __forceinline__ uint32_t gf_mul4(uint32_t v, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
        p ^= v & bit_mask(b, k);
        v = ((v & 0x7F7F7F7Fu) << 1) ^ (((v >> 7) & 0x01010101u) * 0x87u);
    }
    return p;
}
__device__ __forceinline__ uint32_t gf_sq(uint32_t a) { return gf_mul(a, a); }
// a^254 = 1 / a (a != 0)
__device__ __forceinline__ uint32_t gf_inv(uint32_t a)
{
    uint32_t p = 1, s = a;
#pragma unroll
    for (uint32_t k = 1; k < 8; ++k) { s = gf_sq(s); p = gf_mul(p, s); }      // a^(2 + 4 + ... + 128)
    return p;
}
// a^111 (111 = 64 + 32 + 8 + 4 + 2 + 1)
__device__ __forceinline__ uint32_t gf_pow111(uint32_t a)
{
    const uint32_t a2 = gf_sq(a), a4 = gf_sq(a2), a8 = gf_sq(a4), a16 = gf_sq(a8), a32 = gf_sq(a16), a64 = gf_sq(a32);
    return gf_mul(gf_mul(gf_mul(a, a2), gf_mul(a4, a8)), gf_mul(a32, a64));
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, (int)o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, (int)o, 64));
    return v;
}
__device__ __forceinline__ uint32_t lane_get(uint32_t v, uint32_t l) { return (uint32_t)__shfl((int)v, (int)l, 64); }
__device__ __forceinline__ uint32_t count_lanes(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// The 32 syndromes of the word in wb[1 .. 255]: lane l returns that of root l & 31.
__device__ __forceinline__ uint32_t syndromes(const uint8_t* wb, const SsdvTables* tab, uint32_t lane)
{
    const uint32_t m = lane & 31u, half = lane >> 5;
    uint32_t c[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) c[k] = tab->rootmul[m][k];
    // lanes 0 .. 31: bytes 1 .. 128; lanes 32 .. 63: bytes 129 .. 255 behind a zero
    const uint32_t j0 = half ? 128u : 1u;
    uint32_t s = 0;
    for (uint32_t t = 0; t < 128; ++t) {
        uint32_t p = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) p ^= c[k] & bit_mask(s, k);
        const uint32_t b = wb[j0 + t];
        s = p ^ ((half && t == 0) ? 0u : b);
    }
    if (!half) s = gf_mul(s, tab->root127[m]);
    return s ^ (uint32_t)__shfl_xor((int)s, 32, 64);
}

// CRC-32 of wb[1 .. 219] against wb[220 .. 223] (every lane the same work: the addresses are the wave's)
__device__ __forceinline__ bool crc_ok(const uint8_t* wb)
{
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 1; i <= 219; ++i) {
        c ^= wb[i];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    c = ~c;
    const uint32_t have = (uint32_t)wb[220] << 24 | (uint32_t)wb[221] << 16 | (uint32_t)wb[222] << 8 | wb[223];
    return uni32(c) == uni32(have);
}

}  // namespace

__global__ __launch_bounds__(kSsdvAppendTile) void k_ssdv_append(const SsdvSrc* __restrict__ src, const uint32_t* __restrict__ stage, uint32_t* ring_all,
                                                                  size_t ring_stride)
{
    const uint32_t s = blockIdx.y;
    const uint32_t n = min(uni32(src[s].stage_n), kSsdvRing), at = uni32(src[s].stage_at);
    const uint32_t k = blockIdx.x * kSsdvAppendTile + threadIdx.x;
    if (k >= n) return;
    uint32_t* ring = ring_all + (size_t)s * ring_stride + kSsdvGuard;
    ring[((uint32_t)uni64(src[s].append_pos) + k) & kMask] = stage[at + k];
}

__global__ __launch_bounds__(kSsdvWaves * 64) void k_ssdv_scan(const SsdvSrc* __restrict__ src, const SsdvTables* __restrict__ tab,
                                                               const uint32_t* __restrict__ ring_all, size_t ring_stride, uint32_t* cnt,
                                                               SsdvOut* __restrict__ out, uint32_t out_cap)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kSsdvWaves][256];
    const uint32_t lane = threadIdx.x & 63u, wave = uni32(threadIdx.x >> 6);
    const uint32_t s = blockIdx.y;
    const uint32_t idx = blockIdx.x * kSsdvWaves + wave;
    if (idx >= uni32(src[s].n)) return;                              // (a whole wave leaves: nothing below waits for another wave)
    const uint64_t pos = uni64(src[s].base) + uni32(src[s].off) + idx;
    const uint32_t* ring = ring_all + (size_t)s * ring_stride + kSsdvGuard;
    uint8_t* wb = lds[wave];

    // the candidate's words: position j = lane + 64 q
    uint32_t word[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) word[q] = ring[((uint32_t)pos + lane + 64u * q) & kMask];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) wb[lane + 64u * q] = (uint8_t)word[q];
    wave_lds_sync();

    uint32_t trial = 0, errors = 0, erasures = 0, changed = 0, bad = 0;
    bool accepted = false;

    if (uni32(wb[0]) == 0x55u && uni32(wb[1]) == HD_SSDV_TYPE_NOFEC && crc_ok(wb)) { accepted = true; trial = HD_SSDV_NOFEC; }

    uint32_t syn = 0;
    if (!accepted) {
        syn = syndromes(wb, tab, lane);
        if (__ballot(syn != 0) == 0) {                               // a codeword as it stands: every trial finds it
            if (crc_ok(wb)) accepted = true;
            else bad = 4;
        } else {
            uint32_t key[4], rank4 = 0xFFFFFFFFu, era_x = 0;         // rank4: byte q is the position's place among the 24 smallest keys, 255: not among them
            uint32_t gam = lane == 0 ? 1u : 0u;                      // the erasure locator so far
            for (uint32_t t = 0; t < 4 && !accepted; ++t) {
                const uint32_t f = 8u * t;
                if (t == 1) {
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) key[q] = (lane + 64u * q) ? ((word[q] & ~0xFFu) | (lane + 64u * q)) : 0xFFFFFFFFu;
                    for (uint32_t i = 0; i < 24; ++i) {
                        const uint32_t mn = uni32(wave_min(min(min(key[0], key[1]), min(key[2], key[3]))));
#pragma unroll
                        for (uint32_t q = 0; q < 4; ++q)
                            if (key[q] == mn && (lane + 64u * q)) { key[q] = 0xFFFFFFFFu; rank4 = (rank4 & ~(0xFFu << (8u * q))) | (i << (8u * q)); }
                        const uint32_t x = tab->loc[mn & 0xFFu];
                        if (lane == i) era_x = x;
                    }
                }
                for (uint32_t i = f ? f - 8u : 0u; i < f; ++i) {     // gam *= (1 + X_i x)
                    const uint32_t x = uni32(lane_get(era_x, i));
                    const uint32_t up = lane_up(gam, 1);
                    gam ^= gf_mul(lane ? up : 0u, x);
                }
                // Berlekamp-Massey from the erasure locator on, without an inverse: lam is a multiple of the locator
                uint32_t lam = gam, B = gam, L = f, gamma = 1;
                for (uint32_t r = f + 1; r <= 32; ++r) {
                    const uint32_t sv = lane < r ? lane_get(syn, (r - 1u - lane) & 31u) : 0u;
                    const uint32_t d = uni32(wave_xor(gf_mul(lam, sv)));
                    const uint32_t up = lane_up(B, 1), xB = lane ? up : 0u;
                    if (d == 0) { B = xB; continue; }
                    const uint32_t T = gf_mul(lam, gamma) ^ gf_mul(xB, d);
                    if (2u * L <= r + f - 1u) { L = r + f - L; B = lam; gamma = d; }
                    else B = xB;
                    lam = T;
                }
                const uint64_t nz = __ballot(lam != 0);
                if (!nz) continue;
                const uint32_t deg = 63u - (uint32_t)__clzll(nz);
                if (deg > 32u || deg < f || 2u * (deg - f) + f > 32u) continue;
                // the roots: byte q of acc is lam at 1 / loc[lane + 64 q]
                uint32_t acc = 0;
                for (uint32_t k = 0; k <= deg; ++k) acc ^= gf_mul4(tab->chien[k][lane], uni32(lane_get(lam, k)));
                bool root[4];
                uint32_t roots = 0;
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    root[q] = ((acc >> (8u * q)) & 0xFFu) == 0 && (lane + 64u * q) != 0;
                    roots += count_lanes(root[q]);
                }
                if (roots != deg) continue;
                // omega = syn * lam mod x^32, coefficient i on lane i
                uint32_t om = 0;
                for (uint32_t k = 0; k <= deg; ++k) {
                    const uint32_t lk = uni32(lane_get(lam, k));
                    const uint32_t sv = lane_get(syn, (lane - k) & 31u);
                    if (lane < 32u && k <= lane) om ^= gf_mul(sv, lk);
                }
                bool broken = false;
                uint32_t e = 0, ch = 0;
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t j = lane + 64u * q;
                    uint32_t y = 0;
                    if (__ballot(root[q])) {
                        const uint32_t xi = tab->loc[255u - j], x2 = gf_sq(xi);
                        uint32_t num = 0, den = 0, p2 = 1;
                        for (uint32_t k = 32; k > 0; --k) num = gf_mul(num, xi) ^ uni32(lane_get(om, k - 1u));
                        for (uint32_t k = 1; k <= deg; k += 2) { den ^= gf_mul(p2, uni32(lane_get(lam, k))); p2 = gf_mul(p2, x2); }
                        if (root[q]) {
                            if (den == 0) broken = true;
                            else y = gf_mul(gf_mul(num, gf_pow111(xi)), gf_inv(den));
                        }
                    }
                    const bool erased = ((rank4 >> (8u * q)) & 0xFFu) < f;
                    e += count_lanes(y != 0 && !erased);
                    ch += count_lanes(y != 0 && erased);
                    wb[j] = (uint8_t)((word[q] & 0xFFu) ^ y);
                }
                wave_lds_sync();
                if (__ballot(broken) || 2u * e + f > 32u) continue;
                const uint32_t s2 = syndromes(wb, tab, lane);
                if (__ballot(s2 != 0)) continue;
                if (!crc_ok(wb)) { bad += 1; continue; }
                accepted = true; trial = t; errors = e; erasures = f; changed = ch;
            }
        }
    }

    if (bad && lane == 0) atomicAdd(cnt + 1u + s, bad);
    if (!accepted) return;
    uint32_t slot = 0;
    if (lane == 0) slot = atomicAdd(cnt, 1u);
    slot = uni32(slot);
    if (slot >= out_cap) return;                                     // (cannot be: hd_ssdv_create refuses more streams than out_cap, so a launch has at most out_cap candidates)
    wave_lds_sync();
    SsdvOut* o = out + slot;
    uint32_t w4 = reinterpret_cast<const uint32_t*>(wb)[lane];
    if (lane == 0) {
        w4 = (w4 & ~0xFFu) | 0x55u;
        o->pos = pos; o->stream = s; o->trial = trial; o->errors = errors; o->erasures = erasures; o->changed = changed; o->_pad = 0;
    }
    o->data[lane] = w4;
}

void launch_ssdv_append(hipStream_t st, uint32_t n_streams, uint32_t max_n, const SsdvSrc* src, const uint32_t* stage, uint32_t* ring, size_t ring_stride)
{
    if (!n_streams || !max_n) return;
    k_ssdv_append<<<dim3((max_n + kSsdvAppendTile - 1) / kSsdvAppendTile, n_streams), dim3(kSsdvAppendTile), 0, st>>>(src, stage, ring, ring_stride);
}

void launch_ssdv_scan(hipStream_t st, uint32_t n_streams, uint32_t cap, const SsdvSrc* src, const SsdvTables* tab, const uint32_t* ring, size_t ring_stride,
                      uint32_t* cnt, SsdvOut* out, uint32_t out_cap)
{
    if (!n_streams || !cap) return;
    k_ssdv_scan<<<dim3((cap + kSsdvWaves - 1) / kSsdvWaves, n_streams), dim3(kSsdvWaves * 64), 0, st>>>(src, tab, ring, ring_stride, cnt, out, out_cap);
}

}  // namespace hd
