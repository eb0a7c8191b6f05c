// What the side objects' kernels (baud_probe.hip, clocked.hip, tones.hip, tone_search.hip) ask of a wave of 64 lanes beside their own arithmetic.
#pragma once
#include <hip/hip_runtime.h>

namespace hd {

// a value every lane holds alike, said so to the compiler: it moves into scalar registers
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return ((uint64_t)uni32((uint32_t)(v >> 32)) << 32) | uni32((uint32_t)v); }

// Inclusive scan over the wave, T = uint32_t or uint64_t: lane l gets the sum of lanes 0 .. l, mod 2^32 or 2^64; lane_up is v of the lane o below.
// (k_clocked and k_waterfall_detect keep the 32-bit scan written out: from here it is the same operation, but their code comes out with other registers.)
__device__ __forceinline__ uint32_t lane_up(uint32_t v, uint32_t o) { return (uint32_t)__shfl_up((int)v, o, 64); }
__device__ __forceinline__ uint64_t lane_up(uint64_t v, uint32_t o) { return ((uint64_t)lane_up((uint32_t)(v >> 32), o) << 32) | lane_up((uint32_t)v, o); }
template <typename T>
__device__ __forceinline__ T wave_scan(T v, uint32_t lane)
{
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const T up = lane_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

}  // namespace hd
