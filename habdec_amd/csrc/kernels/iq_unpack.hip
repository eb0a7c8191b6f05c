// Packed IQ in front of stage 1 (hd_process_*_fmt, hd_survey_push_*_fmt; include/habdec_amd.h: HD_IQ_*): k_iq_unpack expands rows of little-endian
// cs16 / cs8 / cu8 samples (I then Q) into the engine's cf32 staging slabs, and every kernel behind it runs as on a cf32 push.  Not in the reference:
// its sources convert on the host, sample by sample.
//
//   cs16: (float)v * 2^-15      cs8: (float)v * 2^-7      cu8: (float)(2 v - 255) * 2^-8   (centre 127.5)
//
// Every value is an integer of at most 16 bits times a power of two: exact in float whatever the instruction sequence, so this file has one
// arithmetic (not compiled per mode) and the host model (host/iq_convert.hpp) agrees with it bit for bit.
//
// Shape: grid (tiles, rows), 256 threads.  A row's bytes [row, row + n bps) split at the 16-byte boundaries of its ADDRESS into a head of fewer
// than 16 bytes, whole 16-byte vectors and a tail; a cs16 row may start on any 4-byte boundary and a cs8 / cu8 row on any 2-byte boundary.  Thread t
// of the row owns vector t: one 16-byte load (a wave reads 1 KiB contiguous) and 32 (cs16: 4 samples) or 64 (cs8 / cu8: 8 samples) contiguous
// bytes of the destination, in 16-byte stores: where the row's vectors land 8 bytes off a 16-byte boundary (an odd head in a 16-byte aligned
// row), the thread's first and last sample go alone and the pairs between them are aligned again.  Head and tail samples go one per thread through loads of exactly one sample in the row's first tile:
// no byte outside the row is read, nothing behind sample n of the destination row is written.  No LDS, no atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include "../../../include/habdec_amd.h"
#include "../host/iq_convert.hpp"
#include "launch.h"

namespace hd {

namespace {

template <int FMT>
__device__ __forceinline__ float2 iq_one(const uint32_t w)      // the sample in the low 8 * bps bits of w
{
    if constexpr (FMT == HD_IQ_CS16) {
        return make_float2((float)(int)(int16_t)(w & 0xFFFFu) * 0x1p-15f, (float)(int)(int16_t)(w >> 16) * 0x1p-15f);
    } else if constexpr (FMT == HD_IQ_CS8) {
        return make_float2((float)(int)(int8_t)(w & 0xFFu) * 0x1p-7f, (float)(int)(int8_t)((w >> 8) & 0xFFu) * 0x1p-7f);
    } else {
#ifdef HD_IQ_MUTANT_CENTRE128
        return make_float2((float)(2 * (int)(w & 0xFFu) - 256) * 0x1p-8f, (float)(2 * (int)((w >> 8) & 0xFFu) - 256) * 0x1p-8f);
#else
        return make_float2((float)(2 * (int)(w & 0xFFu) - 255) * 0x1p-8f, (float)(2 * (int)((w >> 8) & 0xFFu) - 255) * 0x1p-8f);
#endif
    }
}

template <int FMT>
__device__ __forceinline__ float2 iq_load_one(const unsigned char* p)    // exactly one sample's bytes
{
    uint32_t w;
    if constexpr (FMT == HD_IQ_CS16) w = *reinterpret_cast<const uint32_t*>(p);
    else w = *reinterpret_cast<const uint16_t*>(p);
    float2 v = iq_one<FMT>(w);
#ifdef HD_IQ_MUTANT_SWAP
    v = make_float2(v.y, v.x);
#endif
    return v;
}

// One plain 16-byte store of two samples, p 16-byte aligned.  Spelled out: written as float4 assignments in the two branches below, the stores are merged
// across the branches component by component and come out as pieces of 4 and 12 bytes.  (s_nop 1: a store of more than 8 bytes reads its data
// registers late; the compiler does not see the store and may schedule a write to them right behind it.)
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store16(float2* p, const float2 a, const float2 b)
{
    const f32x4_t q = {a.x, a.y, b.x, b.y};
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(p), "v"(q) : "memory");
}

template <int FMT>
__device__ __forceinline__ void iq_unpack_body(const unsigned char* __restrict__ src, const size_t src_stride, const uint32_t* __restrict__ n_per_row,
                                               const uint32_t n_uniform, float2* __restrict__ dst, const size_t dst_stride)
{
    constexpr uint32_t kBps = FMT == HD_IQ_CS16 ? 4u : 2u;          // bytes per sample
    constexpr uint32_t kSpv = 16u / kBps;                           // samples per 16-byte vector
    const uint32_t row = blockIdx.y;
    const uint32_t n = n_per_row ? n_per_row[row] : n_uniform;
    const unsigned char* s = src + (size_t)row * src_stride * kBps;
    float2* d = dst + (size_t)row * dst_stride;
    uint32_t head = (uint32_t)((16u - ((uint32_t)reinterpret_cast<uintptr_t>(s) & 15u)) & 15u) / kBps;   // samples in front of the first 16-byte boundary
    head = head < n ? head : n;
    const uint32_t nvec = (n - head) / kSpv, tail = (n - head) - nvec * kSpv;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;

    if (blockIdx.x == 0) {                                          // head: threads [0, 8), tail: threads [8, 16) of the row's first tile
        const uint32_t l = threadIdx.x;
#ifndef HD_IQ_MUTANT_NO_HEAD
        if (l < head) d[l] = iq_load_one<FMT>(s + (size_t)l * kBps);
#endif
        if (l >= 8u && l - 8u < tail) {
            const uint32_t i = head + nvec * kSpv + (l - 8u);
            d[i] = iq_load_one<FMT>(s + (size_t)i * kBps);
        }
    }
    if (t >= nvec) return;
    const uint4 w = *reinterpret_cast<const uint4*>(s + (size_t)head * kBps + (size_t)t * 16u);
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
    float2 v[kSpv];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        if constexpr (FMT == HD_IQ_CS16) v[i] = iq_one<FMT>(ww[i]);
        else { v[2 * i] = iq_one<FMT>(ww[i] & 0xFFFFu); v[2 * i + 1] = iq_one<FMT>(ww[i] >> 16); }
    }
#ifdef HD_IQ_MUTANT_SWAP
#pragma unroll
    for (uint32_t i = 0; i < kSpv; ++i) v[i] = make_float2(v[i].y, v[i].x);
#endif
    float2* o = d + head + (size_t)t * kSpv;
    if (!(reinterpret_cast<uintptr_t>(d + head) & 15u)) {           // (uniform over the row) the thread's samples start on a 16-byte boundary
#pragma unroll
        for (uint32_t i = 0; i < kSpv; i += 2) store16(o + i, v[i], v[i + 1]);
    } else {                                                        // ... or 8 bytes behind one: the first and the last sample alone, 16-byte stores between them
        o[0] = v[0];
#pragma unroll
        for (uint32_t i = 1; i + 1 < kSpv; i += 2) store16(o + i, v[i], v[i + 1]);
        o[kSpv - 1] = v[kSpv - 1];
    }
}

}  // namespace

// fmt is uniform over the launch: one kernel, the format's body picked by a scalar branch
__global__ __launch_bounds__(256) void k_iq_unpack(const unsigned char* __restrict__ src, const size_t src_stride, const uint32_t* __restrict__ n_per_row,
                                                   const uint32_t n_uniform, float2* __restrict__ dst, const size_t dst_stride, const int fmt)
{
    if (fmt == HD_IQ_CS16) iq_unpack_body<HD_IQ_CS16>(src, src_stride, n_per_row, n_uniform, dst, dst_stride);
    else if (fmt == HD_IQ_CS8) iq_unpack_body<HD_IQ_CS8>(src, src_stride, n_per_row, n_uniform, dst, dst_stride);
    else iq_unpack_body<HD_IQ_CU8>(src, src_stride, n_per_row, n_uniform, dst, dst_stride);
}

bool launch_iq_unpack(hipStream_t st, int fmt, uint32_t n_rows, uint32_t max_n, const void* src, size_t src_stride, const uint32_t* n_per_row,
                      uint32_t n_uniform, float2* dst, size_t dst_stride)
{
    if (fmt != HD_IQ_CS16 && fmt != HD_IQ_CS8 && fmt != HD_IQ_CU8) return false;
    if (!n_rows || !max_n) return true;
    const uint32_t bps = (uint32_t)iq_bytes(fmt), spv = 16u / bps, tiles = (max_n / spv + 255u) / 256u;   // (a row shorter than a vector still has its head / tail tile)
    const unsigned char* s = static_cast<const unsigned char*>(src);
    for (uint32_t r0 = 0; r0 < n_rows; r0 += 65535u) {              // (rows are the grid's y)
        const uint32_t rows = n_rows - r0 < 65535u ? n_rows - r0 : 65535u;
        hipLaunchKernelGGL(k_iq_unpack, dim3(tiles ? tiles : 1u, rows), dim3(256), 0, st, s + (size_t)r0 * src_stride * bps, src_stride,
                           n_per_row ? n_per_row + r0 : nullptr, n_uniform, dst + (size_t)r0 * dst_stride, dst_stride, fmt);
    }
    return true;
}

}  // namespace hd
