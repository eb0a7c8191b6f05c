// The LDS image of k_fir_demod (kernels/fir_demod.hip) as a function of the low-pass tap count, and its inverse: pure host arithmetic, no HIP call.
//
// A tile's workgroup keeps [kFirTile outputs' worth of inputs | T taps' worth of history | what whole blocks of sixteen taps read past the last tap | 4]
// complex samples in dynamic LDS, beside kFirStaticLds bytes of static LDS (the two checksum words and their padding).  The image grows with the tap count and a
// workgroup cannot have more LDS than the device grants one, so the longest filter the kernel can run follows from the device: 6611 taps inside
// 64 KB, 18899 inside the 160 KB of a gfx950 CU.  The engine derives its limit from these functions at creation (hd_engine_lowpass_taps_max) and
// refuses a longer design while the call is planned; launch_fir_demod sizes its launch with the same formula.  Lifting the limit is a kernel change
// (a tile loader that walks the taps in pieces).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../dev_types.h"

namespace hd {

constexpr int kFirLanes = 256;
#ifndef HD_FIR_OUT
#define HD_FIR_OUT 6
#endif
constexpr int kFirOut = HD_FIR_OUT;              // adjacent outputs per lane (even; 6: lanes 48 bytes apart, conflict-free 16-byte LDS reads)
constexpr int kFirTile = kFirOut * kFirLanes;    // outputs computed per tile
constexpr int kFirAdvance = kFirTile - kFirOut;  // outputs written per tile (lane 0 only supplies lane 1's predecessor)
constexpr int kFirWin = (16 + kFirOut) / 2;      // 16-byte pairs a block of sixteen taps touches (samples 0 .. 14 + kFirOut of the lane's window)
constexpr int kFirSlack = 16 + 2 * kFirWin;      // samples a lane may read past its last tap (the re-read last block of a kFirOut-output window)
static_assert(kFirOut % 2 == 0 && kFirOut >= 2 && kFirOut <= 8, "outputs per lane: pairs of samples, lane windows 16-byte aligned");

constexpr size_t kFirStaticLds = 16;             // k_fir_demod's static LDS: s_ck[2], padded so that the 16-byte aligned dynamic array starts behind it
                                                 // (tests/test_fir_lds.py holds the compiler's figure for both arithmetic modes against it)
constexpr size_t kFirSampleBytes = 2 * sizeof(float);

// dynamic LDS bytes of a k_fir_demod launch whose longest filter has `taps` taps (0: no stream filters -- the image of one tap)
constexpr size_t fir_demod_lds_bytes(uint32_t taps)
{
    return ((size_t)kFirTile + (taps ? taps : 1u) + (size_t)kFirSlack + 4u) * kFirSampleBytes;
}

// the largest odd tap count (every design is odd, FirFilter.h:185-188) whose launch -- dynamic and static LDS together -- fits `lds_limit` bytes; 0: none does
constexpr uint32_t fir_demod_max_taps(size_t lds_limit)
{
    if (lds_limit < kFirStaticLds + fir_demod_lds_bytes(1)) return 0;
    const size_t n = (lds_limit - kFirStaticLds) / kFirSampleBytes - ((size_t)kFirTile + (size_t)kFirSlack + 4u);
    const size_t odd = (n & 1u) ? n : n - 1u;
    return odd > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)odd;
}

// StreamCall::fir_taps_prev keeps the previous run's tap count in kTapsPrevMax's sixteen bits (dev_types.h): the engine caps its limit there, and on
// today's device the LDS image is what binds long before
static_assert(fir_demod_max_taps(160 * 1024) <= kTapsPrevMax && fir_demod_max_taps(64 * 1024) > 4097, "low-pass tap limit against the fir_taps_prev field");
static_assert(fir_demod_lds_bytes(fir_demod_max_taps(160 * 1024)) + kFirStaticLds <= 160 * 1024 &&
              fir_demod_lds_bytes(fir_demod_max_taps(160 * 1024) + 2) + kFirStaticLds > 160 * 1024, "fir_demod_max_taps inverts fir_demod_lds_bytes");

}  // namespace hd
