// Diversity combiner (hd_combine_*, include/habdec_amd.h has the definition): one group in plain C++, sample by sample and lag by lag, and what the
// engine object and this restatement share -- the parameter rules and the align step.  Not in the reference.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../../include/habdec_amd.h"

namespace hd {

inline void combine_lag_params_default(hd_combine_lag_params* p) { *p = hd_combine_lag_params{8192u, 2048u, 0u, 76u, 16u}; }

inline bool combine_lag_params_ok(const hd_combine_lag_params* p)
{
    return p->window >= HD_COMBINE_MIN_WINDOW && p->window <= HD_COMBINE_MAX_WINDOW && p->window % 64u == 0 && p->max_lag >= 64u &&
           p->max_lag <= HD_COMBINE_MAX_LAG && p->max_lag % 64u == 0 && p->guard >= 1u;
}

// (the clocked decoder's rule)
inline int32_t combine_quantise(float v)
{
    if (v != v) return 0;
    return (int32_t)(std::min(std::max(v, -4.0f), 4.0f) * 1024.0f);
}

// The align step behind a search: res[0] is the reference's entry.  Valid members get delay = top - lag, top the largest valid lag and 0; invalid ones get
// weight 0 and keep their delay.  Returns how many entries are valid, the reference's among them.
inline int combine_align(const hd_combine_lag* res, uint32_t count, uint32_t* delay, uint32_t* weight)
{
    int32_t top = 0;
    int valid = 0;
    for (uint32_t m = 0; m < count; ++m) if (res[m].valid) { top = std::max(top, res[m].lag); ++valid; }
    for (uint32_t m = 0; m < count; ++m) {
        if (res[m].valid) delay[m] = (uint32_t)(top - res[m].lag);
        else weight[m] = 0;
    }
    return valid;
}

struct CombineHostGroup {
    uint32_t count = 0;
    uint32_t stream[HD_COMBINE_MAX_MEMBERS] = {}, delay[HD_COMBINE_MAX_MEMBERS] = {}, weight[HD_COMBINE_MAX_MEMBERS] = {};
    uint64_t n = 0;
    std::vector<int16_t> ring[HD_COMBINE_MAX_MEMBERS];
    std::vector<int32_t> scores;                 // [count - 1][2 L + 1] of the last search
    uint32_t scores_L = 0;

    bool make(const uint32_t* streams, uint32_t k)
    {
        if (!streams || k < 1 || k > HD_COMBINE_MAX_MEMBERS) return false;
        for (uint32_t a = 0; a < k; ++a) for (uint32_t b = 0; b < a; ++b) if (streams[a] == streams[b]) return false;
        count = k;
        for (uint32_t m = 0; m < k; ++m) { stream[m] = streams[m]; delay[m] = 0; weight[m] = 256; ring[m].assign(HD_COMBINE_RING, 0); }
        n = 0;
        return true;
    }
    void reset() { n = 0; scores.clear(); scores_L = 0; }

    // rows[m * stride + j]: member m's sample j of the push; out: n floats
    void push(const float* rows, size_t stride, size_t len, float* out)
    {
        int64_t wt = 0;
        for (uint32_t m = 0; m < count; ++m) wt += weight[m];
        wt = std::max<int64_t>(wt, 1);
        for (size_t j = 0; j < len; ++j, ++n) {
            int64_t sum = 0;
            for (uint32_t m = 0; m < count; ++m) {
                ring[m][n % HD_COMBINE_RING] = (int16_t)combine_quantise(rows[m * stride + j]);
                if (n >= delay[m]) sum += (int64_t)weight[m] * ring[m][(n - delay[m]) % HD_COMBINE_RING];
            }
            out[j] = (float)(int32_t)(sum / wt) / 1024.0f;
        }
    }

    // HD_ERR_INVALID: the parameters; HD_ERR_UNSUPPORTED: fewer than N + 2 L samples.  out: count entries.
    int lags(const hd_combine_lag_params* p, hd_combine_lag* out)
    {
        if (!combine_lag_params_ok(p)) return HD_ERR_INVALID;
        const uint64_t N = p->window, L = p->max_lag;
        if (n < N + 2 * L) return HD_ERR_UNSUPPORTED;
        scores.assign((size_t)(count - 1) * (2 * L + 1), 0);
        scores_L = (uint32_t)L;
        out[0] = hd_combine_lag{stream[0], 0, (int32_t)N, 0, 1u};
        std::vector<uint8_t> br(N), bm(N + 2 * L);
        for (uint64_t i = 0; i < N; ++i) br[i] = ring[0][(n - L - N + i) % HD_COMBINE_RING] > 0;
        for (uint32_t m = 1; m < count; ++m) {
            for (uint64_t i = 0; i < N + 2 * L; ++i) bm[i] = ring[m][(n - N - 2 * L + i) % HD_COMBINE_RING] > 0;
            int32_t* sc = scores.data() + (size_t)(m - 1) * (2 * L + 1);
            for (int64_t l = -(int64_t)L; l <= (int64_t)L; ++l) {
                const uint8_t* b = bm.data() + (L + l);
                int32_t agree = 0;
                for (uint64_t i = 0; i < N; ++i) agree += br[i] == b[i];
                sc[l + (int64_t)L] = 2 * agree - (int32_t)N;
            }
            int32_t lag = 0, peak = INT32_MIN;
            for (int64_t l = -(int64_t)L; l <= (int64_t)L; ++l) {
                const int32_t s = sc[l + (int64_t)L];
                const bool better = s > peak || (s == peak && (std::llabs(l) < std::abs(lag) || (std::llabs(l) == std::abs(lag) && l < lag)));
                if (better) { peak = s; lag = (int32_t)l; }
            }
            int32_t second = -(int32_t)N;
            for (int64_t l = -(int64_t)L; l <= (int64_t)L; ++l)
                if (std::llabs(l - lag) > (int64_t)p->guard) second = std::max(second, sc[l + (int64_t)L]);
            const bool valid = 256ll * peak >= (int64_t)p->min_peak_q8 * (int64_t)N && 256ll * ((int64_t)peak - second) >= (int64_t)p->min_margin_q8 * (int64_t)N;
            out[m] = hd_combine_lag{stream[m], lag, peak, second, valid ? 1u : 0u};
        }
        return HD_OK;
    }
};

}  // namespace hd
