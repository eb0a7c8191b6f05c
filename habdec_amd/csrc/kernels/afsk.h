// AFSK / AX.25 (hd_afsk_*, include/habdec_amd.h): the launchers of kernels/afsk.hip.  The layouts both sides agree on are host/afsk_state.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/habdec_amd.h"
#include "../host/afsk_state.hpp"
#include "launch.h"

namespace hd {

// Slot kernel, one workgroup per stream.  src[s] (the clocked decoder's descriptor): of the n_total floats of the push this launch takes the n from
// index off on (n <= cap <= HD_AFSK_CHUNK; n = 0, or a stream without a modem: not touched).  st [S]; ring32 [S][4][ring32_stride] uint32, a stream's
// four rings of kAfskRing32 running sums, each behind kAfskGuard guard words; ctab: the probe's cosine table; slots [S][slot_stride] int32,
// HD_AFSK_RING records behind kAfskGuard guard words.  cap: the longest n of the launch, which sizes the LDS; false: more than the CU has.
bool launch_afsk_slots(hipStream_t st, uint32_t n_streams, uint32_t cap, const ClockedSrc* src, AfskState* state, uint32_t* ring32, size_t ring32_stride,
                       const int32_t* ctab, int32_t* slots, size_t slot_stride);

// The dynamic LDS of such a launch in bytes; 0 for a cap launch_afsk_slots refuses.
uint32_t afsk_slots_lds_bytes(uint32_t cap);

// Gate, one workgroup per stream.  gate[s]: see AfskGate; count [S] behind kAfskGuard guard words; list [S][list_stride] uint32, list_cap offsets
// behind kAfskGuard guard words, in increasing order whatever the launch's geometry.
void launch_afsk_gate(hipStream_t st, uint32_t n_streams, const AfskGate* gate, const int32_t* slots, size_t slot_stride, uint32_t* count, uint32_t* list,
                      size_t list_stride, uint32_t list_cap);

// Frame kernel, one wave per candidate.  cand[s]: see AfskCand; out: out_cap records, record out_off + k the k-th of the stream's part.  Grid (cap, the
// longest n of the launch; S).
void launch_afsk_frames(hipStream_t st, uint32_t n_streams, uint32_t cap, const AfskCand* cand, const AfskPatterns* pat, uint32_t require_addr,
                        const int32_t* slots, size_t slot_stride, const uint32_t* list, size_t list_stride, hd_afsk_candidate* out, uint32_t out_cap);

}  // namespace hd
