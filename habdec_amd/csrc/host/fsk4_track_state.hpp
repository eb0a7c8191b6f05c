// The 4FSK tone tracker's layouts (hd_fsk4_track_*, include/habdec_amd.h): one set of structs for kernels/fsk4_track.hip and its restatement
// host/fsk4_track.hpp.
#pragma once
#include <cstdint>

namespace hd {

constexpr uint32_t kFsk4CombBins = 4096;           // HD_TONE_SEARCH_BINS: the tone search's spectrum
constexpr uint32_t kFsk4TrackGuard = 16, kFsk4TrackGuardWord = 0x4F5C7A4Bu;   // guard words around every accumulator, carry buffer and record

// A stream's search in integers (host/fsk4_track.hpp: fsk4_comb_plan): the window w (odd, >= 3), the spacings d_lo .. d_hi in quarter bins, the band
// b_lo .. b_hi in bins, known: the spacing is given (d_lo == d_hi) and only f0 is fitted.  Every d has a candidate:
// b_lo + 2 (w / 2) + ((3 d_hi + 2) >> 2) <= b_hi <= 4095.
struct Fsk4CombPlan {
    uint32_t w, d_lo, d_hi, b_lo, b_hi, known;
};
// src[s] of a comb launch: due = 0, the stream is not touched.  segments_ok: the stream has min_segments effective segments.  Behind the record the
// stream's sums are multiplied by decay_q8 / 256.
struct Fsk4CombSrc {
    Fsk4CombPlan plan;
    uint32_t due, min_quality_q8, segments_ok, decay_q8, _pad[2];
};

}  // namespace hd
