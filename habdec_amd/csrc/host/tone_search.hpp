// Host side of the tone search (hd_tone_search_*, include/habdec_amd.h): the detector that turns a stream's long-averaged power spectrum into its two
// FSK tones, and one stream of the spectrum itself in plain C++ with a double-precision transform -- what the CPU suite holds the definition to.
// Pure functions and a small class, no GPU; exported as hd_host_tone_search_* (include/habdec_amd_host.h).  Not in the reference.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/habdec_amd.h"
#include "survey.hpp"

namespace hd {

constexpr uint32_t kToneSearchBins = HD_TONE_SEARCH_BINS, kToneSearchHop = HD_TONE_SEARCH_HOP;
static_assert(kToneSearchBins == HD_SURVEY_BINS && kToneSearchHop == HD_SURVEY_HOP, "the tone search uses the survey's segment, window and transform");

inline void tone_search_detect_params_default(hd_tone_search_detect_params* p) { p->baud = 0.0; p->shift_lo_hz = 170.0; p->shift_hi_hz = 1000.0; p->min_quality = 0.5; }

// The detector, in the order of the header's description (habdec_amd_host.h).  power[i] belongs to f = (i - 2048) fsd / 4096.  All sums sequential, ascending.
inline int tone_search_detect(const double* P, uint64_t segments, double fsd, const hd_tone_search_detect_params* p, hd_tone_search_result* out)
{
    constexpr int N = (int)kToneSearchBins;
    if (out) *out = hd_tone_search_result{};
    if (!P || !p || !out) return HD_ERR_INVALID;
    if (!(p->baud > 0.0) || !(fsd > 0.0) || std::isinf(p->baud) || std::isinf(fsd)) return HD_ERR_INVALID;
    if (!(p->shift_lo_hz > 0.0) || !(p->shift_hi_hz >= p->shift_lo_hz) || std::isinf(p->shift_hi_hz) || !(p->min_quality >= 0.0)) return HD_ERR_INVALID;
    if (segments < 8) return HD_ERR_UNSUPPORTED;
    const double bin = fsd / (double)N;
    // 1. the tone's width in bins, odd
    const double wd = std::max(1.0, std::nearbyint(0.5 * p->baud / bin));
    if (!(wd < (double)N)) return HD_ERR_INVALID;                     // (no pair of windows fits: the same answer as a shift_hi that leaves no d)
    const int w = (int)wd | 1, h = w / 2;
    // 2. the spacings searched
    const double dlo = std::ceil(p->shift_lo_hz / bin), dhi = std::floor(p->shift_hi_hz / bin);
    const int d1 = (int)std::min(dhi, (double)(N - w));
    if (!(dlo >= 1.0) || dlo > (double)d1) return HD_ERR_INVALID;
    const int d0 = (int)dlo;
    out->w = (uint32_t)w; out->segments = segments;
    // 3. a non-finite power: nothing is searched (the stream took a NaN or an Inf; hd_tone_search_reset clears it)
    for (int i = 0; i < N; ++i) if (!std::isfinite(P[i])) return HD_OK;
    // 4. the floor: the median
    std::vector<double> sorted(P, P + N);
    std::sort(sorted.begin(), sorted.end());
    const double floor = 0.5 * (sorted[N / 2 - 1] + sorted[N / 2]);
    out->floor = floor;
    // 5. the power above the floor in a window of w bins around k
    std::vector<double> B(N, 0.0);
    for (int k = h; k < N - h; ++k) {
        double s = 0.0;
        for (int m = k - h; m <= k + h; ++m) s += P[m] - floor;
        B[k] = s;
    }
    // 6. the coarse search: both windows must hold power, so the pair's score is the weaker one's
    double score = -HUGE_VAL;
    int best_lo = h, best_d = d0;
    for (int d = d0; d <= d1; ++d)
        for (int lo = h; lo <= N - h - d - 1; ++lo) {
            const double sc = std::min(B[lo], B[lo + d]);
            if (sc > score) { score = sc; best_lo = lo; best_d = d; }
        }
    out->bin_lo = (uint32_t)best_lo; out->shift_bins = (uint32_t)best_d;
    // 7. refinement: three rounds of a centroid over +-r bins of each tone
    const int r = (int)std::max(1.0, std::nearbyint(0.3 * p->baud / bin));
    double f[2];
    for (int t = 0; t < 2; ++t) {
        int c = t ? best_lo + best_d : best_lo;
        double cf = (double)c;
        for (int round = 0; round < 3; ++round) {
            double sw = 0.0, sm = 0.0;
            for (int m = std::max(c - r, 0); m <= std::min(c + r, N - 1); ++m) {
                const double wt = std::max(P[m] - floor, 0.0);
                sw += wt; sm += (double)m * wt;
            }
            cf = sw > 0.0 ? sm / sw : (double)c;
            c = (int)std::nearbyint(cf);
        }
        f[t] = (cf - (double)(N / 2)) * bin;
    }
    out->f_lo_hz = f[0]; out->f_hi_hz = f[1];
    // 8. quality and validity
    const double quality = floor > 0.0 ? score / ((double)w * floor) : 0.0;
    out->quality = quality;
    out->valid = floor > 0.0 && quality >= std::max(p->min_quality, 10.0 / std::sqrt((double)w * (double)segments)) ? 1u : 0u;
    return HD_OK;
}

// One stream of the spectrum: the segmentation over the absolute sample index, the float window table with one rounded float product per part, then a
// double-precision radix-2 transform, |X|^2 in double, the half swap and the double accumulators.
struct ToneSearchStream {
    std::vector<float> win;
    std::vector<std::complex<double>> tw;         // W4096^m, m < 2048
    std::vector<std::complex<float>> carry;       // the samples from 2048 * segments on: at most 4095 after a push
    std::vector<double> acc;
    uint64_t segments = 0, samples = 0;
    double sum_w2 = 0;
    ToneSearchStream() : win(kToneSearchBins), tw(kToneSearchBins / 2), acc(kToneSearchBins, 0.0)
    {
        survey_window(win.data());
        for (float v : win) sum_w2 += (double)v * (double)v;
        const double two_pi = 2.0 * 3.14159265358979323846264338327950288;
        for (uint32_t m = 0; m < kToneSearchBins / 2; ++m) tw[m] = {std::cos(two_pi * m / kToneSearchBins), -std::sin(two_pi * m / kToneSearchBins)};
    }
    void reset() { carry.clear(); std::fill(acc.begin(), acc.end(), 0.0); segments = samples = 0; }
    void segment(const std::complex<float>* x)
    {
        constexpr uint32_t N = kToneSearchBins;
        std::vector<std::complex<double>> a(N);
        for (uint32_t n = 0; n < N; ++n) {                                         // bit-reversed order in, natural order out
            uint32_t rv = 0;
            for (uint32_t b = 0; b < 12; ++b) rv |= ((n >> b) & 1u) << (11 - b);
            const float re = x[n].real() * win[n], im = x[n].imag() * win[n];      // one rounded float product per part
            a[rv] = {(double)re, (double)im};
        }
        for (uint32_t len = 2; len <= N; len <<= 1) {
            const uint32_t half = len / 2, step = N / len;
            for (uint32_t i = 0; i < N; i += len)
                for (uint32_t j = 0; j < half; ++j) {
                    const std::complex<double> wv = tw[j * step], u = a[i + j], v = a[i + j + half];
                    const std::complex<double> t(v.real() * wv.real() - v.imag() * wv.imag(), v.real() * wv.imag() + v.imag() * wv.real());
                    a[i + j] = u + t; a[i + j + half] = u - t;
                }
        }
        for (uint32_t k = 0; k < N; ++k) acc[(k + N / 2) & (N - 1)] += a[k].real() * a[k].real() + a[k].imag() * a[k].imag();
        ++segments;
    }
    void push(const float* iq, size_t n)
    {
        const std::complex<float>* x = reinterpret_cast<const std::complex<float>*>(iq);
        carry.insert(carry.end(), x, x + n);
        samples += n;
        size_t at = 0;
        for (; carry.size() - at >= kToneSearchBins; at += kToneSearchHop) segment(carry.data() + at);
        carry.erase(carry.begin(), carry.begin() + (ptrdiff_t)at);
    }
    // p[k] = acc[k] / (segments sum w^2); zeros without a segment
    void power(double* p) const
    {
        const double norm = (double)segments * sum_w2;
        for (uint32_t i = 0; i < kToneSearchBins; ++i) p[i] = segments ? acc[i] / norm : 0.0;
    }
};

}  // namespace hd
