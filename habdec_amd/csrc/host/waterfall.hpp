// Host side of the waterfall (hd_waterfall_*, include/habdec_amd.h): the row detector in plain C++ -- what k_waterfall_detect computes, bit for bit --,
// the tracker that links the rows' marks into tracks, and the parameter defaults.  Pure functions, no GPU; exported as hd_host_waterfall_*
// (include/habdec_amd_host.h).  Not in the reference.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/habdec_amd.h"

namespace hd {

inline void waterfall_params_default(hd_waterfall_params* p) { p->slot_segments = 16; p->rows_cap = 1024; p->threshold_db = 6.0; p->dc_guard_hz = 0.0; }
inline void waterfall_track_params_default(hd_waterfall_track_params* p) { p->merge_hz = 1500.0; p->max_width_hz = 0.0; p->gap_rows = 1; p->min_rows = 3; }

// F[s]: the level over the floor for a row of s segments; computed in double, rounded to float once
inline float waterfall_factor(double threshold_db, uint32_t s) { return (float)std::max(std::pow(10.0, threshold_db / 10.0), 1.0 + 8.0 / std::sqrt((double)s)); }

// The bins the guard takes out, [lo, hi): those with |f_i| < dc_guard_hz, f_i = (i - 2048) fs / 4096 (the survey's expression).  false: no bin is left.
inline bool waterfall_guard_range(double fs, double dc_guard_hz, uint32_t* lo, uint32_t* hi)
{
    constexpr uint32_t N = HD_SURVEY_BINS;
    const double binw = fs / (double)N;
    uint32_t a = N, b = 0;
    for (uint32_t i = 0; i < N; ++i)
        if (dc_guard_hz > 0.0 && std::fabs(((double)i - (double)(N / 2)) * binw) < dc_guard_hz) { a = std::min(a, i); b = i + 1; }
    if (a == N) a = b = 0;
    *lo = a; *hi = b;
    return b - a < N;
}

inline bool waterfall_params_ok(const hd_waterfall_params* p)
{
    return p->slot_segments >= 16 && p->slot_segments <= HD_SURVEY_RUN && p->rows_cap >= 1 && p->threshold_db >= 0.0 && p->dc_guard_hz >= 0.0;   // (NaN compares false)
}

// The detector on one row, in the order of the header's description.  Every float operation is rounded once.  Writes hdr->segments, flags, floor,
// level, n_marked (first_sample and _pad = 0) and the 128 mark words.  p->slot_segments and p->rows_cap are not looked at.
inline int waterfall_detect_row(const float* row, uint32_t segments, double fs, const hd_waterfall_params* p, hd_waterfall_row* hdr, uint32_t* marks)
{
    constexpr uint32_t N = HD_SURVEY_BINS;
    if (!row || !p || !hdr || !marks || !(fs > 0)) return HD_ERR_INVALID;
    if (segments < 1 || segments > HD_SURVEY_RUN || !(p->threshold_db >= 0.0) || !(p->dc_guard_hz >= 0.0)) return HD_ERR_INVALID;
    uint32_t g0, g1;
    if (!waterfall_guard_range(fs, p->dc_guard_hz, &g0, &g1)) return HD_ERR_INVALID;
    std::memset(hdr, 0, sizeof *hdr);
    std::memset(marks, 0, HD_WATERFALL_WORDS * sizeof(uint32_t));
    hdr->segments = segments;
    if (segments < 16) hdr->flags |= HD_WF_SHORT;
    // 1. bit patterns
    std::vector<uint32_t> key(N);
    std::memcpy(key.data(), row, N * sizeof(float));
    for (uint32_t i = 0; i < N; ++i) if (key[i] > 0x7F800000u) { hdr->flags |= HD_WF_BAD; return HD_OK; }
    // 2., 3. the floor: the median of the eligible values, ordered as unsigned patterns
    std::vector<uint32_t> s;
    s.reserve(N);
    for (uint32_t i = 0; i < N; ++i) if (i < g0 || i >= g1) s.push_back(key[i]);
    std::sort(s.begin(), s.end());
    auto as_float = [](uint32_t u) { float f; std::memcpy(&f, &u, sizeof f); return f; };
    const size_t m = s.size();
    float floor;
    if (m & 1) floor = as_float(s[m / 2]);
    else { const float sum = as_float(s[m / 2 - 1]) + as_float(s[m / 2]); floor = 0.5f * sum; }
    if (floor == 0.0f || std::isinf(floor)) { hdr->flags |= HD_WF_NO_FLOOR; return HD_OK; }
    // 4. the level
    const float level = floor * waterfall_factor(p->threshold_db, segments);
    hdr->floor = floor; hdr->level = level;
    if (hdr->flags) return HD_OK;                                       // (a short row: floor and level, no marks)
    // 5. marks
    for (uint32_t i = 0; i < N; ++i)
        if ((i < g0 || i >= g1) && row[i] >= level) { marks[i >> 5] |= 1u << (i & 31); ++hdr->n_marked; }
    return HD_OK;
}

// The tracker: headers[n_rows], marks[n_rows][128] -> tracks, in the order of the header's description.
inline int waterfall_tracks(const hd_waterfall_row* headers, const uint32_t* marks, uint64_t n_rows, double fs, const hd_waterfall_track_params* p,
                            hd_waterfall_track* out, uint32_t cap, uint32_t* found)
{
    constexpr uint32_t N = HD_SURVEY_BINS;
    if (found) *found = 0;
    if (!p || !found || (cap && !out) || !(fs > 0) || (n_rows && (!headers || !marks))) return HD_ERR_INVALID;
    if (!(p->merge_hz >= 0.0) || !(p->max_width_hz >= 0.0)) return HD_ERR_INVALID;
    const double binw = fs / (double)N;
    const double gd = std::ceil(p->merge_hz / binw);
    const uint32_t g = gd >= (double)N ? N : (uint32_t)gd;
    struct Trk { hd_waterfall_track t; uint64_t sum_idx; };
    std::vector<Trk> open, done;
    struct Cl { uint32_t lo, hi, n; uint64_t sum; };
    std::vector<Cl> cl;
    for (uint64_t r = 0; r < n_rows; ++r) {
        // 2. the row's clusters (a flagged row has none)
        cl.clear();
        if (headers[r].flags == 0) {
            const uint32_t* mw = marks + r * HD_WATERFALL_WORDS;
            for (uint32_t i = 0; i < N; ++i) {
                if (!((mw[i >> 5] >> (i & 31)) & 1u)) continue;
                if (cl.empty() || i - cl.back().hi - 1 > g) cl.push_back({i, i, 0, 0});
                cl.back().hi = i; ++cl.back().n; cl.back().sum += i;
            }
        }
        // 3. a cluster joins the first open track it touches, else opens one
        for (const Cl& c : cl) {
            Trk* hit = nullptr;
            for (Trk& k : open)
                if (c.lo <= k.t.bin_hi + g && c.hi + g >= k.t.bin_lo) { hit = &k; break; }
            if (!hit) {
                Trk k{};
                k.t.first_row = r; k.t.last_row = r; k.t.first_sample = headers[r].first_sample; k.t.rows_hit = 1;
                k.t.bin_lo = c.lo; k.t.bin_hi = c.hi; k.t.marks = c.n; k.sum_idx = c.sum;
                open.push_back(k);
                continue;
            }
            if (hit->t.last_row != r) { ++hit->t.rows_hit; hit->t.last_row = r; }
            hit->t.bin_lo = std::min(hit->t.bin_lo, c.lo); hit->t.bin_hi = std::max(hit->t.bin_hi, c.hi);
            hit->t.marks += c.n; hit->sum_idx += c.sum;
        }
        // 4. tracks that have been silent for more than gap_rows rows are closed
        for (size_t k = 0; k < open.size();) {
            if (r - open[k].t.last_row > p->gap_rows) { done.push_back(open[k]); open.erase(open.begin() + (ptrdiff_t)k); }
            else ++k;
        }
    }
    for (Trk& k : open) { k.t.open = 1; done.push_back(k); }
    std::vector<hd_waterfall_track> res;
    for (Trk& k : done) {
        hd_waterfall_track& t = k.t;
        t.end_sample = headers[t.last_row].first_sample + ((uint64_t)headers[t.last_row].segments + 1) * HD_SURVEY_HOP;
        t.offset_hz = ((double)k.sum_idx / (double)t.marks - (double)(N / 2)) * binw;
        t.width_hz = (double)(t.bin_hi - t.bin_lo + 1) * binw;
        if (t.rows_hit < p->min_rows) continue;
        if (p->max_width_hz > 0.0 && t.width_hz > p->max_width_hz) continue;
        res.push_back(t);
    }
    std::stable_sort(res.begin(), res.end(), [](const hd_waterfall_track& a, const hd_waterfall_track& b) {
        return a.first_sample != b.first_sample ? a.first_sample < b.first_sample : a.offset_hz < b.offset_hz;
    });
    *found = (uint32_t)res.size();
    for (uint32_t i = 0; i < std::min<uint32_t>(*found, cap); ++i) out[i] = res[i];
    return HD_OK;
}

}  // namespace hd
