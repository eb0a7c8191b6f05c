// The pieces of the in-wave spectrum (spectrum_wave.h) that host code shares with the kernels: where a 64-point transform leaves its bins, the
// lane-major twiddle table, and the per-bin division by the sampling rate.  Plain C++ as well as HIP: tests/test_spectrum_div.py compiles this
// header with g++.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HD_SPEC_HD __host__ __device__
#else
#define HD_SPEC_HD
#endif

namespace hd {
namespace specwave {

// Where bin k of a 64-point transform sits in the register array after fft64 (8 x 8 decomposition, second-level output k2 left in its
// row): X[k1 + 8 k2] = a[8 k1 + k2].
constexpr int xpos(int k) { return 8 * (k & 7) + (k >> 3); }

// The factors between the two passes of the 4096-point transform, the way the wave reads them: lane l holds pass 1's bin k1 = xpos(i) in register i
// and multiplies it by W4096^(l k1), so tw64[i][l] = tw4096[(l * xpos(i)) & 4095] with tw4096[m] = (cos, -sin)(2 pi m / 4096) rounded once from
// double.  Register i of the whole wave is then one contiguous 512-byte row.  F2: any pair with float members x and y.
template <class F2>
inline void fft_twiddles(F2* tw64 /* [64][64] */)
{
    float tw4096[4096][2];
    for (int m = 0; m < 4096; ++m) {
        const double a = 2.0 * 3.14159265358979323846264338327950288 * (double)m / 4096.0;
        tw4096[m][0] = (float)cos(a);
        tw4096[m][1] = (float)-sin(a);
    }
    for (int i = 0; i < 64; ++i)
        for (int l = 0; l < 64; ++l) {
            const int m = (l * xpos(i)) & 4095;
            tw64[64 * i + l].x = tw4096[m][0];
            tw64[64 * i + l].y = tw4096[m][1];
        }
}

// (float)((double)q / rate) for many q and one rate, without the division: t = (double)q * rinv with rinv = 1.0 / rate differs from the exact
// quotient by at most about one part in 2^52 (two roundings of 2^-53 each), i.e. by about two units of t's last place, and so does the rounded
// quotient by half a unit.  (float)t is therefore the float the division gives unless a float rounding boundary lies within that distance of t.  For
// a normal float result the boundaries are the doubles whose low 29 significand bits are 0x10000000 (the midpoints between floats): t is taken
// only when its low 29 bits are more than 4 away from that pattern.  Results below the normal floats (other boundaries), zero, Inf and NaN are
// not taken either.
HD_SPEC_HD inline bool spec_div_fast_ok(const double t)
{
    uint64_t b;
    __builtin_memcpy(&b, &t, sizeof b);
    const uint32_t low = (uint32_t)b & 0x1FFFFFFFu;
    return t >= 0x1p-126 && t < (double)INFINITY && low - 0x0FFFFFFCu > 8u;
}

// slow (may be null): set where the division itself was needed
HD_SPEC_HD inline float spec_div(const float q, const double rate, const double rinv, bool* slow = nullptr)
{
    const double t = (double)q * rinv;
    const bool ok = spec_div_fast_ok(t);
    if (slow) *slow = !ok;
    return ok ? (float)t : (float)((double)q / rate);
}

}  // namespace specwave
}  // namespace hd
