// Host side of the per-stream tuning (kernels/tune.h): the phase step of an offset and the two phasor tables.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../kernels/tune.h"

namespace hd {

// step = -(offset / decimated_rate) cycles per sample in units of 2^-32, rounded half to even; false outside (-rate/2, rate/2)
inline bool tune_step(double offset_hz, double decimated_rate, uint32_t* step)
{
    if (!(decimated_rate > 0) || !(std::fabs(offset_hz) < decimated_rate / 2)) return false;
    *step = (uint32_t)(int64_t)std::nearbyint(-(offset_hz / decimated_rate) * 4294967296.0);
    return true;
}

// coarse[2a..2a+1] = (cos, sin)(2 pi a / 256), fine[2b..2b+1] = (cos, sin)(2 pi b / 65536): computed in double, rounded once
inline void tune_tables(float* coarse, float* fine)
{
    const double two_pi = 2.0 * 3.14159265358979323846264338327950288;
    for (uint32_t k = 0; k < kTuneTable; ++k) {
        const double a = two_pi * (double)k / 256.0, b = two_pi * (double)k / 65536.0;
        coarse[2 * k] = (float)std::cos(a); coarse[2 * k + 1] = (float)std::sin(a);
        fine[2 * k] = (float)std::cos(b); fine[2 * k + 1] = (float)std::sin(b);
    }
}

// out[i] = iq[i] * phasor(phase + i * step), interleaved (I, Q); in place allowed
inline void tune_rotate(const float* tab, const float* iq, size_t n, uint32_t phase, uint32_t step, float* out)
{
    uint32_t theta = phase;
    for (size_t i = 0; i < n; ++i, theta += step) tune_rotate1(tab, theta, iq[2 * i], iq[2 * i + 1], out[2 * i], out[2 * i + 1]);
}

}  // namespace hd
