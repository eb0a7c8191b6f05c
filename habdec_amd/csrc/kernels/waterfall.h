// Waterfall (hd_waterfall_*, include/habdec_amd.h): launchers of kernels/waterfall.hip and the record both sides agree on.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace hd {

constexpr uint32_t kWaterfallBins = 4096;      // one row: the survey's 4096 fftshifted bins
constexpr uint32_t kWaterfallWords = 128;      // HD_WATERFALL_WORDS
constexpr uint32_t kWaterfallMaxSeg = 64;      // most segments a row sums (HD_SURVEY_RUN)

// What the detector leaves per row and what crosses the link: 16 bytes of results and the 4096 mark bits (528 bytes)
struct WaterfallRec {
    uint32_t flags;                            // HD_WF_*
    float floor, level;                        // 0 where the flags leave them undefined
    uint32_t n_marked;
    uint32_t marks[kWaterfallWords];           // bit i & 31 of word i >> 5: bin i
};
static_assert(sizeof(WaterfallRec) == 528, "16 bytes of results and 128 mark words");

// One workgroup per row: rows[b][4096] float sums (non-negative or +inf; anything else flags the row HD_WF_BAD) -> out[b].  Row b sums segments[b]
// segments (a device array), or with segments == nullptr seg_full of them, the launch's last row seg_last.  Bins [guard_lo, guard_hi) are not
// eligible (guard_lo == guard_hi: all are); factor[s], s = 1..64, is the level over the floor for a row of s segments (a device table of 65 floats).
void launch_waterfall_detect(hipStream_t st, uint32_t n_rows, const float* rows, const uint32_t* segments, uint32_t seg_full, uint32_t seg_last,
                             uint32_t guard_lo, uint32_t guard_hi, const float* factor, WaterfallRec* out);
// hits[i] += the mark bits of bin i over rec[0 .. n_rows), flagged rows skipped; one thread per bin and 64 rows, integer atomics (n_rows >= 1)
void launch_waterfall_hits(hipStream_t st, const WaterfallRec* rec, uint32_t n_rows, uint32_t* hits);

}  // namespace hd
