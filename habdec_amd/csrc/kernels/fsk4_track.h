// 4FSK tone tracker (hd_fsk4_track_*, include/habdec_amd.h): the launcher of kernels/fsk4_track.hip.  The layouts both sides agree on are
// host/fsk4_track_state.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../host/fsk4_track_state.hpp"

namespace hd {

// Comb detector, one workgroup per stream.  src[s]: see Fsk4CombSrc (due = 0: the stream is not touched).  acc [S][acc_stride] double: a stream's 4096
// fftshifted sums behind kFsk4TrackGuard / 2 guard doubles, as k_tone_search writes them; read, and multiplied by decay_q8 / 256 behind the record.
// rec [S][rec_stride] uint32: a stream's record, the 16 words of hd_fsk4_comb_record, behind kFsk4TrackGuard guard words.
void launch_fsk4_comb(hipStream_t st, uint32_t n_streams, const Fsk4CombSrc* src, double* acc, size_t acc_stride, uint32_t* rec, size_t rec_stride);

}  // namespace hd
