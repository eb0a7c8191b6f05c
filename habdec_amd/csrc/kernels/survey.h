// Wideband survey (hd_survey_*, include/habdec_amd.h): launchers of kernels/survey.hip and the push geometry both sides agree on.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace hd {

constexpr uint32_t kSurveyBins = 4096;     // HD_SURVEY_BINS: one segment, one transform
constexpr uint32_t kSurveyHop = 2048;      // HD_SURVEY_HOP: segment s of a push is samples [2048 s, 2048 s + 4096)
constexpr uint32_t kSurveyRun = 64;        // HD_SURVEY_RUN: most segments one wave sums in float before its row goes out

// whole segments of a push of n samples; segments never straddle pushes, samples behind the last whole hop are not used
inline uint64_t survey_segments(uint64_t n) { return n < kSurveyBins ? 0 : 1 + (n - kSurveyBins) / kSurveyHop; }
// segments per wave of a push: what decides which float sums are formed, so a push cut into several launches keeps the one push's value
inline uint32_t survey_run_len(uint64_t n_seg, uint32_t runs_per_launch)
{
    const uint64_t r = (n_seg + runs_per_launch - 1) / runs_per_launch;
    return (uint32_t)(r < kSurveyRun ? (r ? r : 1) : kSurveyRun);
}

// One wave per run: run b of the launch sums segments [seg0 + b run_len, min(seg0 + (b + 1) run_len, n_seg)) of the push at x into partial[b][4096]
// (fftshifted).  win[4096]: the window; tw64: the lane-major twiddle table (spectrum_math.h: fft_twiddles).  Every block must own at least one segment.
void launch_survey(hipStream_t st, uint32_t n_runs, const float2* x, const float* win, const float2* tw64, float* partial, uint64_t seg0, uint64_t n_seg,
                   uint32_t run_len);
// acc[i] += partial[0][i], then partial[1][i], ... partial[n_runs - 1][i], in double, one thread per bin
void launch_survey_reduce(hipStream_t st, const float* partial, uint32_t n_runs, double* acc);

}  // namespace hd
