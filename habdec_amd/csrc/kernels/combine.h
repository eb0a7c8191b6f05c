// Diversity combiner (hd_combine_*, include/habdec_amd.h): the launchers of kernels/combine.hip and the layout both sides agree on.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../dev_types.h"
#include "../../../include/habdec_amd.h"

namespace hd {

constexpr uint32_t kCombineRing = HD_COMBINE_RING;          // a member's newest samples, int16, slot = absolute index & (kCombineRing - 1)
constexpr uint32_t kCombineMembers = HD_COMBINE_MAX_MEMBERS;
// guard words in front of and behind every ring and every output row: kCombineGuard 32-bit words, which is 2 kCombineGuard int16 samples
constexpr uint32_t kCombineGuard = 16, kCombineGuardWord = 0xC0B1E5D7u;
constexpr uint32_t kCombineTile = 256;                      // samples of a chunk per workgroup of k_combine
constexpr uint32_t kCombineLagBlock = 256;                  // lags per workgroup of k_combine_lags: 64 per wave

// src[s]: the clocked decoder's descriptor (launch.h: ClockedSrc) -- of the n_total floats of the push this launch takes the n from index off on; p is
// linear memory, or (ring_mask != 0) the engine's symbol ring, in which the push ends at the append position base + held of *sym.
struct CombineSrc {
    const float* p;
    const SymState* sym;
    uint32_t n_total, ring_mask, off, n;
};
// One group of a launch: its members' streams (the reference first), delays and weights, wt = max(1, the weights' sum), and `base`, the group's sample
// count in front of the PUSH (the absolute index of the push's sample 0): sample off + j of the push has the absolute index base + off + j.
struct CombineGroup {
    uint64_t base;
    uint32_t count, wt;
    uint32_t stream[kCombineMembers], delay[kCombineMembers], weight[kCombineMembers];
};
// ring [S][ring_stride] int16: a stream's kCombineRing samples behind 2 kCombineGuard guard samples; rows [S][row_stride] float: row_cap floats behind
// kCombineGuard guard words.  Grid (n_groups, tiles of kCombineTile samples over cap, the longest n of the launch).
void launch_combine(hipStream_t st, uint32_t n_groups, uint32_t cap, const CombineSrc* src, const CombineGroup* groups, int16_t* ring, size_t ring_stride,
                    float* rows, size_t row_stride, uint32_t row_cap);

// The lag search of one group whose members hold n samples each (n >= N + 2 L, N + 2 L <= kCombineRing: the caller's checks).  scores [count - 1][2 L + 1]
// int32, member m's at (m - 1) * (2 L + 1): score of lag l at index l + L.  out [count - 1]: the members' results behind the reference's.
void launch_combine_lags(hipStream_t st, const CombineGroup* group /* host copy */, uint64_t n, uint32_t N, uint32_t L, uint32_t guard, uint32_t min_peak_q8,
                         uint32_t min_margin_q8, const int16_t* ring, size_t ring_stride, int32_t* scores, hd_combine_lag* out);

}  // namespace hd
