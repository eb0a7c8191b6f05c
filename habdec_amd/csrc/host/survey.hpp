// Host side of the wideband survey (hd_survey_*, include/habdec_amd.h): the window table and the detector that turns the averaged power spectrum
// into candidate payload offsets.  Pure functions, no GPU; exported as hd_host_survey_* (include/habdec_amd_host.h).  Not in the reference.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/habdec_amd.h"

namespace hd {

// periodic Hann, 0.5 - 0.5 cos(2 pi n / 4096): computed in double, rounded to float once
inline void survey_window(float* w)
{
    const double two_pi = 2.0 * 3.14159265358979323846264338327950288;
    for (uint32_t n = 0; n < HD_SURVEY_BINS; ++n) w[n] = (float)(0.5 - 0.5 * std::cos(two_pi * (double)n / (double)HD_SURVEY_BINS));
}

inline void survey_params_default(hd_survey_params* p) { p->threshold_db = 6.0; p->merge_hz = 1500.0; p->dc_guard_hz = 0.0; p->max_width_hz = 0.0; }

// The detector, in the order of the header's description.  power[i] belongs to f = (i - 2048) fs / 4096.
inline int survey_detect(const double* power, uint64_t segments, double fs, const hd_survey_params* p, hd_survey_candidate* out, uint32_t cap, uint32_t* found)
{
    constexpr uint32_t N = HD_SURVEY_BINS;
    if (found) *found = 0;
    if (!power || !p || !found || (cap && !out) || !(fs > 0)) return HD_ERR_INVALID;
    // 1. input checks
    if (segments < 16) return HD_ERR_UNSUPPORTED;
    for (uint32_t i = 0; i < N; ++i) if (!(power[i] >= 0.0)) return HD_ERR_INVALID;                    // (NaN compares false)
    if (!(p->threshold_db >= 0.0) || !(p->merge_hz >= 0.0) || !(p->dc_guard_hz >= 0.0) || !(p->max_width_hz >= 0.0)) return HD_ERR_INVALID;
    const double binw = fs / (double)N;
    auto freq = [&](uint32_t i) { return ((double)i - (double)(N / 2)) * binw; };
    // 2. eligible bins and the floor: their median
    std::vector<uint8_t> eligible(N, 1);
    std::vector<double> sorted;
    sorted.reserve(N);
    for (uint32_t i = 0; i < N; ++i) {
        if (p->dc_guard_hz > 0.0 && std::fabs(freq(i)) < p->dc_guard_hz) eligible[i] = 0;
        else sorted.push_back(power[i]);
    }
    if (sorted.empty()) return HD_ERR_INVALID;                                                          // the guard leaves no bin
    std::sort(sorted.begin(), sorted.end());
    const size_t m = sorted.size();
    const double floor = (m & 1) ? sorted[m / 2] : 0.5 * (sorted[m / 2 - 1] + sorted[m / 2]);
    if (!(floor > 0.0) || std::isinf(floor)) return HD_ERR_UNSUPPORTED;                                 // no floor to hold a threshold against
    // 3. marking
    const double factor = std::max(std::pow(10.0, p->threshold_db / 10.0), 1.0 + 8.0 / std::sqrt((double)segments));
    const double level = floor * factor;
    // 4. clusters: runs of marked bins with at most g unmarked bins between neighbours; no wrap-around
    const double gd = std::ceil(p->merge_hz / binw);
    const uint32_t g = gd >= (double)N ? N : (uint32_t)gd;
    std::vector<hd_survey_candidate> cl;
    bool open = false;
    double sw = 0, sfw = 0;
    uint32_t lo = 0, hi = 0;
    auto close = [&]() {
        hd_survey_candidate c;
        c.offset_hz = sfw / sw;
        c.snr_db = 10.0 * std::log10(sw / floor);
        c.width_hz = (double)(hi - lo + 1) * binw;
        c.bin_lo = lo; c.bin_hi = hi;
        if (!(p->max_width_hz > 0.0 && c.width_hz > p->max_width_hz)) cl.push_back(c);                 // 5. (too wide: dropped)
        open = false;
    };
    for (uint32_t i = 0; i < N; ++i) {
        if (!eligible[i] || !(power[i] >= level)) continue;
        if (open && i - hi - 1 > g) close();
        if (!open) { open = true; lo = i; sw = 0; sfw = 0; }
        hi = i;
        const double w = power[i] - floor;
        sw += w; sfw += freq(i) * w;
    }
    if (open) close();
    // 6. order and output
    std::stable_sort(cl.begin(), cl.end(), [](const hd_survey_candidate& a, const hd_survey_candidate& b) {
        return a.snr_db != b.snr_db ? a.snr_db > b.snr_db : a.offset_hz < b.offset_hz;
    });
    *found = (uint32_t)cl.size();
    for (uint32_t i = 0; i < std::min<uint32_t>(*found, cap); ++i) out[i] = cl[i];
    return HD_OK;
}

}  // namespace hd
