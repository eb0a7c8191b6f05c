// CRC-guided repair of a sentence match whose CRC16 fails (hd_clocked_*, include/habdec_amd.h has the rule): flip the least confident data bits of the
// span, few at a time, until the span is a sentence again and its CRC agrees.  A pure function of the span's characters and soft values; no GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "sentence.hpp"

namespace hd {

constexpr uint32_t kChaseMaxBits = 16, kChaseMaxFlips = 4;

// the sentence scan on `span` alone matches all of it, and the CRC16 agrees
inline bool chase_span_ok(const std::string& span, SentenceMatch& m)
{
    if (span.empty() || span[0] != '$' || !extract_sentence(span, m)) return false;
    if (m.rest.size() != 1) return false;                            // (the scan leaves the CRC's last character behind: the match ends with the span)
    return m.crc == crc16_ccitt_hex(m.callsign + "," + m.data);
}

// span[n], data[n][8] (data_k of every character), nbits 7 or 8.  Returns the number of flipped bits (1 .. max_flips) with `out` and `m` the repaired span
// and its match, or 0: no trial counts.
inline uint32_t chase_repair(const std::string& span, const int32_t* data, uint32_t nbits, uint32_t n_weak, uint32_t max_flips, std::string& out,
                             SentenceMatch& m)
{
    n_weak = std::min(n_weak, kChaseMaxBits); max_flips = std::min(max_flips, kChaseMaxFlips);
    if (!n_weak || !max_flips || span.empty() || nbits < 1 || nbits > 8) return 0;
    struct Weak { uint32_t mag, c, k; };
    std::vector<Weak> all;
    all.reserve(span.size() * nbits);
    for (uint32_t c = 0; c < span.size(); ++c)
        for (uint32_t k = 0; k < nbits; ++k) {
            const int64_t v = data[(size_t)c * 8 + k];
            all.push_back({(uint32_t)(v < 0 ? -v : v), c, k});
        }
    const uint32_t w = (uint32_t)std::min<size_t>(n_weak, all.size());
    std::partial_sort(all.begin(), all.begin() + w, all.end(), [](const Weak& a, const Weak& b) {
        return a.mag != b.mag ? a.mag < b.mag : a.c != b.c ? a.c < b.c : a.k < b.k;
    });
    uint32_t idx[kChaseMaxFlips];
    for (uint32_t size = 1; size <= std::min(max_flips, w); ++size) {
        for (uint32_t i = 0; i < size; ++i) idx[i] = i;              // the subsets of `size` list entries in lexicographic order
        for (;;) {
            out = span;
            bool printable = true;
            for (uint32_t i = 0; i < size; ++i) out[all[idx[i]].c] = (char)((unsigned char)out[all[idx[i]].c] ^ (1u << all[idx[i]].k));
            for (uint32_t i = 0; i < size; ++i) {
                const unsigned char ch = (unsigned char)out[all[idx[i]].c];
                printable &= ch >= 32 && ch <= 126;
            }
            if (printable && chase_span_ok(out, m)) return size;
            int i = (int)size - 1;
            while (i >= 0 && idx[i] == w - size + (uint32_t)i) --i;
            if (i < 0) break;
            ++idx[i];
            for (uint32_t j = (uint32_t)i + 1; j < size; ++j) idx[j] = idx[j - 1] + 1;
        }
    }
    return 0;
}

}  // namespace hd
