// Tone search (hd_tone_search_*, include/habdec_amd.h): the launcher of kernels/tone_search.hip and the layout both sides agree on.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace hd {

constexpr uint32_t kToneSearchSeg = 4096;      // HD_TONE_SEARCH_BINS: one segment, one transform
constexpr uint32_t kToneSearchStep = 2048;     // HD_TONE_SEARCH_HOP: segment j of a stream is its samples [2048 j, 2048 j + 4096)
// guard words in front of and behind every accumulator row and every carry buffer: kToneSearchGuard 32-bit words, which is kToneSearchGuard / 2 doubles
// or cf32 samples, so a row behind its guard keeps a 64-byte alignment
constexpr uint32_t kToneSearchGuard = 16, kToneSearchGuardWord = 0x705EA2C4u;

// whole segments that `carry` samples kept from before and n new ones complete
inline uint32_t tone_search_segments(uint32_t carry, uint32_t n)
{
    const uint64_t have = (uint64_t)carry + n;
    return have < kToneSearchSeg ? 0u : (uint32_t)(1 + (have - kToneSearchSeg) / kToneSearchStep);
}

// One wave per stream.  src[s]: of the n_total cf32 samples of the push at p this launch takes the n from index off on (n = 0: the stream is not touched);
// in front of them lie the `carry` samples of the stream's carry buffer `flip` (0 or 1), and together they complete `segs` segments
// (tone_search_segments(carry, n): the host's count, which the kernel's reads rely on).  The samples from 2048 segs on, carry + n - 2048 segs <= 4095
// of them, are the stream's carry afterwards: in the other buffer when segs > 0, appended in place when segs = 0.
struct ToneSearchSrc {
    const float2* p;
    uint32_t n_total, off, n, carry, segs, flip;
};
// acc [S][acc_stride] double: a stream's 4096 fftshifted sums behind kToneSearchGuard / 2 guard doubles; carry [S][2][carry_stride] cf32: its two carry
// buffers of 4096 samples, each behind kToneSearchGuard / 2 guard samples.  win[4096]: the window; tw64: the lane-major twiddle table
// (spectrum_math.h: fft_twiddles).
void launch_tone_search(hipStream_t st, uint32_t n_streams, const ToneSearchSrc* src, const float* win, const float2* tw64, double* acc, size_t acc_stride,
                        float2* carry, size_t carry_stride);

}  // namespace hd
