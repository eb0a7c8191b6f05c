// Host side of the baud-rate probe (hd_baud_probe_*, include/habdec_amd.h): the candidate tables, the restatement of kernels/baud_probe.hip sample by
// sample, and the estimate that reads a stream's accumulators.  Plain C++, no GPU; exported as hd_host_baud_probe_* (include/habdec_amd_host.h).  Not in
// the reference, which is told its baud rate.
//
// From the first comparison on everything is integer arithmetic: the accumulators are the same bits whatever the order of the sums, so the kernel is
// held to this file bit for bit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/habdec_amd.h"

namespace hd {

constexpr uint32_t kProbeCand = HD_PROBE_CANDIDATES, kProbeScales = HD_PROBE_SCALES;
constexpr uint32_t kProbeW[kProbeScales] = {1, 3, 7, 15, 31, 63, 127, 255, 511};
constexpr uint32_t kProbeEdgeCap = 4096, kProbeEdgeMin = 8, kProbeMinBlocks = 4;
constexpr double kProbeNominal[] = {45.45, 50, 75, 100, 110, 134.5, 150, 200, 300, 600, 1200};

inline void baud_probe_params_default(hd_baud_probe_params* p) { p->baud_lo = 40.0; p->baud_hi = 1300.0; p->min_coherence = 0.5; }

inline bool baud_probe_params_ok(const hd_baud_probe_params* p, double fsd)
{
    return p && fsd > 0 && p->baud_lo > 0 && p->baud_lo < p->baud_hi && p->baud_hi <= fsd / 3.5 && p->min_coherence >= 0;     // (NaN compares false)
}

struct BaudProbeTables {
    double b[kProbeCand];               // candidate baud rates, ascending
    uint32_t F[kProbeCand];             // phase step per sample, 2^-32 cycle (b <= fsd / 3.5: fits 32 bits)
    uint8_t scale[kProbeCand];          // index into kProbeW of the scale the candidate listens to: non-increasing in k
    uint32_t k_lo[kProbeScales], k_hi[kProbeScales];   // the candidates of a scale: [k_lo, k_hi), empty when equal
    int32_t C[1024];                    // nearbyint(32767 cos(2 pi a / 1024))
    double log_step;                    // ln(b[k + 1] / b[k])

    void make(double fsd, const hd_baud_probe_params& p)
    {
        const double two_pi = 2.0 * 3.14159265358979323846264338327950288;
        for (uint32_t a = 0; a < 1024; ++a) C[a] = (int32_t)std::nearbyint(32767.0 * std::cos(two_pi * (double)a / 1024.0));
        for (uint32_t s = 0; s < kProbeScales; ++s) k_lo[s] = k_hi[s] = 0;
        for (uint32_t k = 0; k < kProbeCand; ++k) {
            b[k] = p.baud_lo * std::pow(p.baud_hi / p.baud_lo, (double)k / (double)(kProbeCand - 1));
            F[k] = (uint32_t)(uint64_t)std::floor(b[k] / fsd * 4294967296.0 + 0.5);
            const double lim = std::max(1.0, 4294967296.0 / (double)F[k] / 4.0);
            uint32_t s = 0;
            while (s + 1 < kProbeScales && (double)kProbeW[s + 1] <= lim) ++s;
            scale[k] = (uint8_t)s;
        }
        for (uint32_t k = 0; k < kProbeCand; ++k) {     // (F ascends, so a scale's candidates are one run)
            if (k == 0 || scale[k] != scale[k - 1]) k_lo[scale[k]] = k;
            k_hi[scale[k]] = k + 1;
        }
        log_step = std::log(p.baud_hi / p.baud_lo) / (double)(kProbeCand - 1);
    }
};

inline void baud_probe_dump(hd_baud_probe_candidate& c)
{
    if (c.n >= kProbeEdgeMin && c.n <= kProbeEdgeCap) {
        c.P += (uint64_t)((int64_t)c.re * c.re) + (uint64_t)((int64_t)c.im * c.im);
        c.Q += (uint64_t)c.n * c.n;
        c.NB += 1;
    }
    c.re = c.im = 0;
    c.n = 0;
}

inline void baud_probe_edge(hd_baud_probe_candidate& c, uint64_t i, uint32_t F, const int32_t* C)
{
    const uint64_t p = i * (uint64_t)F;
    const uint32_t idx = (uint32_t)(p >> 22) & 1023u, block = (uint32_t)(p >> 38);
    if (block != c.cur_block) { baud_probe_dump(c); c.cur_block = block; }
    c.n += 1;
    if (c.n <= kProbeEdgeCap) { c.re += C[idx]; c.im += C[(idx + 768u) & 1023u]; }
}

// One stream of the probe.  The history is circular by absolute sample index: bit (j & 63) of word ((j >> 6) & 7) is the sign bit of the newest sample
// j' <= i - 1 with j' = j mod 512, zero before the stream's first sample.
struct BaudProbeStream {
    hd_baud_probe_stream_state h{};
    std::vector<hd_baud_probe_candidate> c;
    uint32_t cnt[kProbeScales] = {};        // popcount of the newest W sign bits (derived from the history)

    BaudProbeStream() : c(kProbeCand) { reset(); }
    void reset()
    {
        std::memset(&h, 0, sizeof h);
        h.n_candidates = kProbeCand;
        std::memset(c.data(), 0, c.size() * sizeof(hd_baud_probe_candidate));
        std::memset(cnt, 0, sizeof cnt);
    }
    uint32_t bit(uint64_t j) const { return (uint32_t)(h.history[(j >> 6) & 7] >> (j & 63)) & 1u; }
    void push(const BaudProbeTables& t, const float* d, size_t n)
    {
        for (size_t x = 0; x < n; ++x) {
            const uint64_t i = h.samples;
            const uint32_t b = d[x] > 0.0f ? 1u : 0u;
            uint64_t& w = h.history[(i >> 6) & 7];
            w = (w & ~(1ull << (i & 63))) | ((uint64_t)b << (i & 63));
            for (uint32_t s = 0; s < kProbeScales; ++s) {
                const uint32_t W = kProbeW[s];
                cnt[s] += b;
                if (i >= W) cnt[s] -= bit(i - W);
                const uint32_t m = cnt[s] > (W - 1) / 2 ? 1u : 0u;
                if (i >= W && m != h.majority[s]) {
                    ++h.edges[s];
                    for (uint32_t k = t.k_lo[s]; k < t.k_hi[s]; ++k) baud_probe_edge(c[k], i, t.F[k], t.C);
                }
                h.majority[s] = m;
            }
            h.samples = i + 1;
        }
    }
};

// The estimate: a pure function of one stream's state.  `cand` is not changed: the open blocks are dumped in a copy.
inline void baud_probe_estimate(const BaudProbeTables& t, const hd_baud_probe_params& prm, const hd_baud_probe_stream_state& h,
                                const hd_baud_probe_candidate* cand, hd_baud_estimate* out)
{
    std::vector<double> rho(kProbeCand);
    double rho_max = 0;
    for (uint32_t k = 0; k < kProbeCand; ++k) {
        hd_baud_probe_candidate c = cand[k];
        baud_probe_dump(c);
        rho[k] = c.NB >= kProbeMinBlocks ? (double)c.P / (32767.0 * 32767.0 * (double)c.Q) : 0.0;
        rho_max = std::max(rho_max, rho[k]);
    }
    uint32_t k = 0;
    while (k + 1 < kProbeCand && !(rho[k] >= 0.5 * rho_max)) ++k;
    while (k + 1 < kProbeCand && rho[k + 1] > rho[k]) ++k;
    double baud = t.b[k];
    if (k > 0 && k + 1 < kProbeCand) {
        const double den = rho[k - 1] - 2.0 * rho[k] + rho[k + 1];
        if (den < 0) {
            const double delta = 0.5 * (rho[k - 1] - rho[k + 1]) / den;
            baud = std::exp(std::log(t.b[k]) + delta * t.log_step);
            baud = std::min(std::max(baud, t.b[k - 1]), t.b[k + 1]);
        }
    }
    double nominal = 0, best = 1e300;
    for (const double nom : kProbeNominal) {
        const double dist = std::fabs(std::log(baud / nom));
        if (dist < best) { best = dist; nominal = nom; }
    }
    if (!(std::fabs(baud / nominal - 1.0) <= 0.015)) nominal = 0;
    std::memset(out, 0, sizeof *out);
    out->baud = baud; out->nominal = nominal; out->rho = rho[k]; out->rho_max = rho_max;
    out->samples = h.samples; out->edges = h.edges[t.scale[k]]; out->k = k;
    out->settled = ((h.samples * (uint64_t)t.F[0]) >> 38) >= 4 ? 1 : 0;
    out->valid = out->settled && rho_max >= prm.min_coherence ? 1 : 0;
}

}  // namespace hd
