// Framing trial: which of 7N1 / 7N2 / 8N1 / 8N2 is a stream of bits?  Four text stages (text_stage.hpp: framer, sentence scan, CRC) over the same
// bits, and the counts that tell them apart.  Host only; exported as hd_host_format_trial_* and teed beside a stream's own text stage by
// hd_stream_set_format_trial.  Not in the reference, which is told its framing.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../../include/habdec_amd.h"
#include "text_stage.hpp"

namespace hd {

struct FormatTrial {
    static constexpr uint32_t kBits[HD_TRIAL_FORMATS] = {7, 7, 8, 8};
    static constexpr float kStops[HD_TRIAL_FORMATS] = {1, 2, 1, 2};
    TextStage t[HD_TRIAL_FORMATS];
    uint64_t matches[HD_TRIAL_FORMATS] = {}, printable[HD_TRIAL_FORMATS] = {};

    FormatTrial() { for (int f = 0; f < HD_TRIAL_FORMATS; ++f) { t[f].framer.nbits = kBits[f]; t[f].framer.nstops = kStops[f]; } }

    void push_bits(const uint8_t* bits, size_t n) { for (auto& s : t) if (n) s.framer.push_bits(bits, n); run(n != 0); }
    void push_packed(const uint32_t* words, uint32_t n) { for (auto& s : t) if (n) s.framer.push_packed(words, n); run(n != 0); }

    void get(hd_format_trial_result* r) const
    {
        std::memset(r, 0, sizeof *r);
        uint64_t top = 0;
        for (int f = 0; f < HD_TRIAL_FORMATS; ++f) {
            r->bits[f] = kBits[f]; r->stops[f] = kStops[f];
            r->sentences_ok[f] = t[f].ok_count; r->matches[f] = matches[f]; r->printable[f] = printable[f];
            top = std::max<uint64_t>(top, t[f].ok_count);
        }
        // A one-stop framer also frames a two-stop signal, and seven data bits read an eight-bit character whose top bit is clear: among the formats
        // that lose no sentence the strictest is the answer -- most stop bits first, then most data bits.
        r->best = -1;
        for (int f = 0; f < HD_TRIAL_FORMATS && top; ++f) {
            if (t[f].ok_count != top) continue;
            if (r->best < 0 || kStops[f] > kStops[r->best] || (kStops[f] == kStops[r->best] && kBits[f] > kBits[r->best])) r->best = f;
        }
        if (r->best >= 0) { r->best_bits = kBits[r->best]; r->best_stops = kStops[r->best]; }
    }

private:
    void run(bool had_bits)
    {
        for (int f = 0; f < HD_TRIAL_FORMATS; ++f) {
            uint64_t& m = matches[f];
            printable[f] += t[f].run(had_bits, [](const SentenceMatch&) {}, [&m](const SentenceMatch&, bool) { ++m; }).size();
            t[f].ok_log.clear(); t[f].match_log.clear(); t[f].char_log.clear();     // (the logs are the C ABI's drains: nobody drains a trial's)
        }
    }
};

}  // namespace hd
