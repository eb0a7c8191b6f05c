// Horus Binary 4FSK (hd_fsk4_*, include/habdec_amd.h): the launchers of kernels/fsk4.hip.  The layouts both sides agree on are host/fsk4_state.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/habdec_amd.h"
#include "../host/fsk4_state.hpp"
#include "launch.h"

namespace hd {

// Slot kernel, one workgroup per stream.  src[s] (the tones object's descriptor): of the n_total cf32 samples of the push at p this launch takes the n
// from index off on (n <= cap <= HD_FSK4_CHUNK; n = 0, or a stream without a modem: not touched).  st [S]; ring32 [S][8][ring32_stride] uint32, a
// stream's eight rings of kFsk4Ring32 running sums, each behind kFsk4Guard guard words; ctab: the probe's cosine table; slots [S][slot_stride] uint32,
// slot_cap records of four words (a power of two) behind kFsk4Guard guard words.  cap: the longest n of the launch, which sizes the LDS; false: more
// than the CU has.
bool launch_fsk4_slots(hipStream_t st, uint32_t n_streams, uint32_t cap, const TonesSrc* src, Fsk4State* state, uint32_t* ring32, size_t ring32_stride,
                       const int32_t* ctab, uint32_t* slots, size_t slot_stride, uint32_t slot_cap);

// Frame kernel, one wave per candidate.  cand[s]: see Fsk4Cand; tab [S]; cnt: the launch's candidates behind the gate (the host clears it in front of a
// launch), behind kFsk4Guard guard words; out: out_cap results.  Grid (cap, the longest n of the launch; S).
void launch_fsk4_frames(hipStream_t st, uint32_t n_streams, uint32_t cap, const Fsk4Cand* cand, const Fsk4Tab* tab, const uint32_t* slots, size_t slot_stride,
                        uint32_t slot_cap, uint32_t uw_max_errors, uint32_t chase_bits, uint32_t* cnt, Fsk4Out* out, uint32_t out_cap);

}  // namespace hd
