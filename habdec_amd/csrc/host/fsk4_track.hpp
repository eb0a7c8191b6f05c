// Host side of the 4FSK tone tracker (hd_fsk4_track_*, include/habdec_amd.h has the definition): the search plan a stream's parameters give, the restatement
// of k_fsk4_comb (kernels/fsk4_track.hip) step by step in the header's order, and one stream of the tracker -- the tone search's double-precision spectrum,
// the epochs, the decay, the records -- with the fsk4 restatement it retunes.  Plain C++, no GPU; exported as hd_host_fsk4_comb_detect and
// hd_host_fsk4_track_* (include/habdec_amd_host.h).  Not in the reference.
//
// Behind the quantisation the detector is integer arithmetic: the kernel's records are held to fsk4_comb_detect byte for byte.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <vector>

#include "../../../include/habdec_amd.h"
#include "fsk4.hpp"
#include "fsk4_track_state.hpp"
#include "tone_search.hpp"

namespace hd {

inline void fsk4_track_params_default(hd_fsk4_track_params* p)
{
    p->max_push = 0; p->epoch_segments = 4; p->decay_q8 = 128; p->min_quality_q8 = 192; p->min_segments = 4; p->deadband = 8;
}
inline bool fsk4_track_params_ok(const hd_fsk4_track_params* p) { return p->epoch_segments >= 1 && p->epoch_segments <= 4096 && p->decay_q8 <= 256; }

// Steps 4, 5 and 8 of the definition in front of the spectrum: the integers of a stream's search.  HD_ERR_UNSUPPORTED: a spacing below 2 baud;
// HD_ERR_INVALID: parameters that are no numbers, or a band and a spacing range that leave no candidate.
inline int fsk4_comb_plan(double fsd, double baud, double spacing_lo, double spacing_hi, double f_lo, double f_hi, Fsk4CombPlan& pl)
{
    constexpr double N = (double)kFsk4CombBins;
    std::memset(&pl, 0, sizeof pl);
    if (!(fsd > 0) || !(baud > 0) || std::isinf(fsd) || std::isinf(baud)) return HD_ERR_INVALID;
    if (!(spacing_lo > 0) || !(spacing_hi >= spacing_lo) || std::isinf(spacing_hi) || !(f_hi > f_lo) || std::isinf(f_lo) || std::isinf(f_hi)) return HD_ERR_INVALID;
    if (spacing_lo < 2.0 * baud) return HD_ERR_UNSUPPORTED;
    const double bin = fsd / N;
    const double wd = std::nearbyint(0.5 * baud / bin);
    if (!(wd < N / 8)) return HD_ERR_INVALID;
    const uint32_t w = std::max<uint32_t>(3u, (uint32_t)wd | 1u), h = w / 2;
    const double blo = std::max(0.0, N / 2 + std::ceil(f_lo / bin)), bhi = std::min(N - 1, N / 2 + std::floor(f_hi / bin));
    if (!(blo <= bhi)) return HD_ERR_INVALID;
    double dlo, dhi;
    if (spacing_lo == spacing_hi) dlo = dhi = std::nearbyint(4.0 * spacing_lo / bin);
    else { dlo = std::ceil(4.0 * spacing_lo / bin); dhi = std::floor(4.0 * spacing_hi / bin); }
    dhi = std::min(dhi, 4.0 * N);
    if (!(dlo >= 4.0) || dlo > dhi) return HD_ERR_INVALID;
    pl.w = w; pl.b_lo = (uint32_t)blo; pl.b_hi = (uint32_t)bhi; pl.d_lo = (uint32_t)dlo; pl.d_hi = (uint32_t)dhi; pl.known = spacing_lo == spacing_hi;
    // the narrowest comb must fit the band: c0 = b_lo + h, its last window's end at c0 + ((3 d_lo + 2) >> 2) + h
    if ((uint64_t)pl.b_lo + 2u * h + ((3u * (uint64_t)pl.d_lo + 2u) >> 2) > pl.b_hi) return HD_ERR_INVALID;
    // (wider ones that do not fit are no candidates; d_hi is cut to the widest that does, so that the kernel's loop bounds say what is searched)
    while (((3u * (uint64_t)pl.d_hi + 2u) >> 2) + pl.b_lo + 2u * h > pl.b_hi) --pl.d_hi;
    return HD_OK;
}

inline int64_t fsk4_floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// Steps 1 .. 9 on 4096 fftshifted sums.
inline void fsk4_comb_detect(const double* acc, const Fsk4CombPlan& pl, uint32_t min_quality_q8, bool segments_ok, hd_fsk4_comb_record* out)
{
    constexpr int N = (int)kFsk4CombBins;
    std::memset(out, 0, sizeof *out);
    // 1
    double mx = 0.0;
    for (int k = 0; k < N; ++k) {
        if (!std::isfinite(acc[k])) return;
        mx = std::max(mx, acc[k]);
    }
    if (!(mx > 0.0)) return;
    // 2
    std::vector<uint32_t> q(N), ps(N + 1, 0u);
    for (int k = 0; k < N; ++k) q[k] = acc[k] > 0.0 ? (uint32_t)std::floor(acc[k] / mx * 524288.0) : 0u;
    for (int k = 0; k < N; ++k) ps[k + 1] = ps[k] + q[k];
    // 3
    std::vector<uint32_t> sorted(q);
    std::nth_element(sorted.begin(), sorted.begin() + (N / 2 - 1), sorted.end());
    const uint32_t floor = sorted[N / 2 - 1];
    // 4, 5
    const int w = (int)pl.w, h = w / 2;
    std::vector<uint32_t> B(N, 0u);                      // the window sum around c
    for (int c = h; c + h < N; ++c) B[c] = ps[c + h + 1] - ps[c - h];
    uint64_t best = 0;
    for (uint32_t d = pl.d_lo; d <= pl.d_hi; ++d) {
        const int o1 = (int)((d + 2u) >> 2), o2 = (int)((2u * d + 2u) >> 2), o3 = (int)((3u * d + 2u) >> 2);
        for (int c0 = (int)pl.b_lo + h; c0 + o3 + h <= (int)pl.b_hi; ++c0) {
            const uint32_t sc = std::min(std::min(B[c0], B[c0 + o1]), std::min(B[c0 + o2], B[c0 + o3]));
            if (sc < (uint32_t)(best >> 32)) continue;
            const uint64_t key = (uint64_t)sc << 32 | (uint64_t)(0xFFFFu - d) << 16 | (uint64_t)(0xFFFFu - (uint32_t)c0);
            if (key > best) best = key;
        }
    }
    if (!best) return;                                   // (no plan of fsk4_comb_plan leaves no candidate)
    const uint32_t score = (uint32_t)(best >> 32), d = 0xFFFFu - (uint32_t)((best >> 16) & 0xFFFFu), c0 = 0xFFFFu - (uint32_t)(best & 0xFFFFu);
    // 6
    int64_t cen[4], sum = 0;
    for (uint32_t t = 0; t < 4; ++t) {
        int64_t c = (int64_t)c0 + ((t * d + 2u) >> 2), cf = 256 * c;
        for (int round = 0; round < 4; ++round) {
            int64_t sw = 0, sm = 0;
            for (int64_t m = std::max<int64_t>(c - w, 0); m <= std::min<int64_t>(c + w, N - 1); ++m) {
                const int64_t wt = q[m] > floor ? (int64_t)(q[m] - floor) : 0;
                sw += wt; sm += (m - c) * wt;
            }
            cf = 256 * c + (sw ? fsk4_floor_div(512 * sm + sw, 2 * sw) : 0);
            c = (cf + 128) >> 8;
        }
        cen[t] = cf; sum += cf;
        out->centroid_q8[t] = (int32_t)cf;
    }
    // 7, 8
    if (pl.known) {
        out->spacing_q8 = (int32_t)(64u * d);
        out->f0_q8 = (int32_t)fsk4_floor_div(sum - 6 * (int64_t)out->spacing_q8 + 2, 4);
    } else {
        const int64_t s10 = -3 * cen[0] - cen[1] + cen[2] + 3 * cen[3];
        out->spacing_q8 = (int32_t)fsk4_floor_div(s10 + 5, 10);
        out->f0_q8 = (int32_t)fsk4_floor_div(5 * sum - 3 * s10 + 10, 20);
    }
    // 9
    const uint64_t wf = (uint64_t)w * floor;
    out->c0 = c0; out->d = d; out->w = (uint32_t)w; out->floor = floor; out->score = score;
    out->quality_q8 = score > wf ? (uint32_t)std::min<uint64_t>(256u * (score - wf) / std::max<uint64_t>(wf, 1u), 0xFFFFFFFFull) : 0u;
    out->valid = out->quality_q8 >= min_quality_q8 && segments_ok ? 1u : 0u;
}

inline double fsk4_track_f0_hz(const hd_fsk4_comb_record& r, double fsd) { return ((double)r.f0_q8 / 256.0 - 2048.0) * (fsd / 4096.0); }
inline double fsk4_track_spacing_hz(const hd_fsk4_comb_record& r, double fsd) { return (double)r.spacing_q8 / 256.0 * (fsd / 4096.0); }

// One stream's epochs, records and counts: what the engine's object and the restatement both run around their spectra.
struct Fsk4TrackBook {
    Fsk4CombPlan plan{};
    double baud = 0;
    bool set = false;
    uint64_t samples = 0, segments = 0, epochs = 0, valid_epochs = 0, retunes = 0;
    double eff = 0;                                  // effective segments
    std::deque<hd_fsk4_track_est> log;
    static constexpr size_t kLog = 4096;

    void reset() { samples = segments = epochs = valid_epochs = retunes = 0; eff = 0; log.clear(); }
    uint64_t epoch_end(uint32_t epoch_segments) const { return 2048u * ((epochs + 1u) * (uint64_t)epoch_segments + 1u); }
    // Samples from `samples` on that end in this epoch: at most `want`, at least 1.
    uint64_t uncut(uint64_t want, uint32_t epoch_segments) const { return std::min<uint64_t>(want, epoch_end(epoch_segments) - samples); }
    // In front of the detector at an epoch's end: the epoch's segments count, and whether the record may be valid.
    bool segments_ok(const hd_fsk4_track_params& p) { eff += (double)p.epoch_segments; return eff >= (double)p.min_segments; }
    // Behind it: the record joins the log, the counts move on, the effective segments decay as the sums do.
    const hd_fsk4_track_est& close_epoch(const hd_fsk4_comb_record& r, const hd_fsk4_track_params& p, double fsd)
    {
        hd_fsk4_track_est e;
        std::memset(&e, 0, sizeof e);
        e.rec = r; e.f0_hz = fsk4_track_f0_hz(r, fsd); e.spacing_hz = fsk4_track_spacing_hz(r, fsd);
        e.end_sample = samples; e.epoch = epochs;
        if (log.size() == kLog) log.pop_front();
        log.push_back(e);
        ++epochs; valid_epochs += r.valid;
        eff *= (double)p.decay_q8 / 256.0;
        return log.back();
    }
    // Closing the loop: does the valid record e ask for a retune of a modem whose steps are phi?  One tone more than deadband / 256 baud away.
    bool wants_retune(const hd_fsk4_track_est& e, const uint32_t* phi, double fsd, uint32_t deadband) const
    {
        if (!e.rec.valid) return false;
        for (uint32_t t = 0; t < 4; ++t) {
            const double have = (double)(int32_t)phi[t] / 4294967296.0 * fsd, want = e.f0_hz + t * e.spacing_hz;
            if (std::fabs(want - have) > (double)deadband / 256.0 * baud) return true;
        }
        return false;
    }
    void stats(hd_fsk4_track_info* o) const { *o = hd_fsk4_track_info{samples, segments, epochs, valid_epochs, retunes}; }
    size_t take_log(hd_fsk4_track_est* out, size_t cap, bool keep)
    {
        if (!out) return log.size();
        const size_t k = std::min(cap, log.size());
        for (size_t i = 0; i < k; ++i) out[i] = log[i];
        if (!keep) log.erase(log.begin(), log.begin() + (ptrdiff_t)k);
        return k;
    }
};

// The steps of the modem whose retunes are all in force: what the tracker compares its estimate with.
inline const uint32_t* fsk4_steps_ahead(const Fsk4Stream& m) { return m.pending.empty() ? m.s.phi : m.pending.back().phi; }

// The restatement: one stream, the tone search's spectrum in double precision.
struct Fsk4TrackStream {
    hd_fsk4_track_params prm{};
    double fsd = 0;
    Fsk4TrackBook book;
    ToneSearchStream ts;
    Fsk4Stream* modem = nullptr;                     // attached: retuned at epoch ends

    void reset() { ts.reset(); book.reset(); }
    void push(const float* iq, size_t n)
    {
        if (!book.set) return;
        for (size_t at = 0; at < n;) {
            const size_t k = (size_t)book.uncut(n - at, prm.epoch_segments);
            ts.push(iq + 2 * at, k);
            at += k;
            book.samples += k; book.segments = ts.segments;
            if (book.samples != book.epoch_end(prm.epoch_segments)) continue;
            hd_fsk4_comb_record r;
            fsk4_comb_detect(ts.acc.data(), book.plan, prm.min_quality_q8, book.segments_ok(prm), &r);
            const double keep = (double)prm.decay_q8 / 256.0;
            for (double& v : ts.acc) v *= keep;
            const hd_fsk4_track_est& e = book.close_epoch(r, prm, fsd);
            if (modem && modem->s.F && book.wants_retune(e, fsk4_steps_ahead(*modem), fsd, prm.deadband)) {
                uint32_t phi[4];
                if (fsk4_retune_steps(fsd, e.f0_hz, e.spacing_hz, phi) == HD_OK) {
                    modem->retune(phi, e.end_sample);
                    modem->apply_retunes();
                    ++book.retunes;
                }
            }
        }
    }
};

}  // namespace hd
