// Host side of the tone-filter demodulator (hd_tones_*, include/habdec_amd.h has the definition): the restatement of kernels/tones.hip sample by sample,
// the parameter checks and the state a reset gives a stream.  Plain C++, no GPU; exported as hd_host_tones_* (include/habdec_amd_host.h).  Not in the
// reference.
//
// Behind the quantisation everything is integer arithmetic: the kernel's rows are held to this file byte for byte.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/habdec_amd.h"
#include "tones_state.hpp"

namespace hd {

inline void tones_params_default(hd_tones_params* p) { p->max_push = 0; p->window_q8 = 160; }
inline bool tones_window_ok(uint32_t window_q8) { return window_q8 >= 32 && window_q8 <= 256; }

// C[a] of the definition: the probe's table
inline void tones_table(int32_t* C)
{
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t a = 0; a < 1024; ++a) C[a] = (int32_t)std::nearbyint(32767.0 * std::cos(two_pi * (double)a / 1024.0));
}

// The state a reset gives a stream with this modem (F = 0: none).
inline void tones_state_reset(TonesState& s, uint32_t F, uint32_t W, uint32_t phi_hi, uint32_t phi_lo)
{
    std::memset(&s, 0, sizeof s);
    s.F = F; s.W = W; s.phi[0] = phi_hi; s.phi[1] = phi_lo;
    s.full = (uint32_t)(((uint64_t)F + 32768u) >> 16);
    s.L = 8u * s.full;
}
inline void tones_state_reset(TonesState& s) { tones_state_reset(s, s.F, s.W, s.phi[0], s.phi[1]); }

// hd_tones_set_modem's checks and the modem's integers: HD_OK and `s` reset with the modem, or the error and `s` untouched.
inline int tones_modem(TonesState& s, double fsd, double baud, double f_hi, double f_lo, uint32_t window_q8)
{
    if (!(fsd > 0) || !(baud > 0) || !tones_window_ok(window_q8)) return HD_ERR_UNSUPPORTED;
    const double spb = fsd / baud;
    if (!(spb >= 3.5 && spb <= (double)HD_TONES_MAX_SPB)) return HD_ERR_UNSUPPORTED;
    if (!(std::fabs(f_hi) < fsd / 2) || !(std::fabs(f_lo) < fsd / 2) || !(f_hi > f_lo)) return HD_ERR_INVALID;
    const uint64_t F = (uint64_t)(int64_t)std::floor(spb * 65536.0 + 0.5);
    const uint64_t W = std::max<uint64_t>(1u, (F * window_q8 + (1u << 23)) >> 24);
    const double two32 = 4294967296.0;
    tones_state_reset(s, (uint32_t)F, (uint32_t)W, (uint32_t)(int64_t)std::nearbyint(f_hi / fsd * two32), (uint32_t)(int64_t)std::nearbyint(f_lo / fsd * two32));
    return HD_OK;
}

inline int32_t tones_quantise(float v)
{
    if (v != v) return 0;
    return (int32_t)(std::min(std::max(v, -8.0f), 8.0f) * 256.0f);
}

// floor(sqrt(x)), x < 2^62: a floating estimate, settled by integer comparisons
inline uint32_t tones_isqrt(uint64_t x)
{
    uint64_t r = (uint64_t)std::sqrt((double)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return (uint32_t)r;
}

// One stream of the demodulator: the state and the rings of running sums, as the kernel keeps them.
struct TonesStream {
    TonesState s{};
    int32_t C[1024];
    std::vector<uint32_t> ring[4];
    std::vector<uint64_t> qring;

    TonesStream() : qring(kTonesRing64, 0u)
    {
        tones_table(C);
        for (auto& r : ring) r.assign(kTonesRing32, 0u);
        tones_state_reset(s, 0, 0, 0, 0);
    }
    void reset() { tones_state_reset(s); }          // (nothing behind index 0 is read: the rings need no clearing)

    // n cf32 samples at iq (re, im interleaved) -> n floats at out; nothing without a modem
    size_t push(const float* iq, size_t n, float* out)
    {
        if (!s.F) return 0;
        for (size_t j = 0; j < n; ++j) {
            const uint64_t i = s.n;
            const int32_t q_re = tones_quantise(iq[2 * j]), q_im = tones_quantise(iq[2 * j + 1]);
            int64_t A[2];
            for (uint32_t t = 0; t < 2; ++t) {
                const uint32_t theta = (uint32_t)i * s.phi[t], a = theta >> 22;
                const int32_t c = C[a], sn = C[(a + 768u) & 1023u];
                const int32_t r[2] = {(q_re * c + q_im * sn) >> 15, (q_im * c - q_re * sn) >> 15};
                int64_t w[2];
                for (uint32_t k = 0; k < 2; ++k) {
                    std::vector<uint32_t>& R = ring[2 * t + k];
                    const uint32_t now = s.tot[2 * t + k] + (uint32_t)r[k];
                    const uint32_t lag = i + 1 <= s.W ? 0u : R[(uint32_t)(i + 1 - s.W) & (kTonesRing32 - 1u)];      // read before the write below: W may be the ring's length
                    R[(uint32_t)(i + 1) & (kTonesRing32 - 1u)] = now;
                    s.tot[2 * t + k] = now;
                    w[k] = (int32_t)(now - lag);
                }
                A[t] = tones_isqrt((uint64_t)(w[0] * w[0] + w[1] * w[1]));
            }
            const uint64_t qnow = s.qtot + (uint64_t)(A[0] + A[1]);
            const uint64_t qlag = i + 1 <= s.L ? 0u : qring[(uint32_t)(i + 1 - s.L) & (kTonesRing64 - 1u)];
            qring[(uint32_t)(i + 1) & (kTonesRing64 - 1u)] = qnow;
            s.qtot = qnow;
            const int64_t N = (int64_t)(qnow - qlag);
            int64_t o = ((A[0] - A[1]) * 1024 * (int64_t)s.L) / std::max<int64_t>(1, N);
            o = std::min<int64_t>(4096, std::max<int64_t>(-4096, o));
            out[j] = (float)o / 1024.0f;
            s.n = i + 1;
        }
        return n;
    }
};

}  // namespace hd
