// Host side of the clocked decoder (hd_clocked_*, include/habdec_amd.h): the restatement of kernels/clocked.hip position by position, and the text stage
// both share -- the sentence scan and CRC of text_stage.hpp over the records' characters, with the repair of chase_repair.hpp where a CRC fails.  Plain
// C++, no GPU; exported as hd_host_clocked_* (include/habdec_amd_host.h).  Not in the reference.
//
// Behind the quantisation everything is integer arithmetic: the kernel's records are held to this file byte for byte.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../../include/habdec_amd.h"
#include "chase_repair.hpp"
#include "clocked_state.hpp"
#include "sentence.hpp"

namespace hd {

static_assert(sizeof(hd_clocked_record) == kClockedRecWords * 4, "hd_clocked_record is 14 words");

inline void clocked_params_default(hd_clocked_params* p) { p->record_cap = 4096; p->repair_bits = 8; p->repair_flips = 3; p->_pad = 0; }
inline bool clocked_params_ok(const hd_clocked_params* p) { return p && p->record_cap >= 16 && p->record_cap <= (1u << 20) && p->repair_bits <= kChaseMaxBits && p->repair_flips <= kChaseMaxFlips; }

// F of the definition, or 0 for a modem hd_clocked_set_modem refuses
inline uint32_t clocked_modem_F(double fsd, double baud, uint32_t nbits, double nstops)
{
    if (!(fsd > 0) || !(baud > 0) || (nbits != 7 && nbits != 8) || (nstops != 1 && nstops != 2)) return 0;
    const double spb = fsd / baud;
    if (!(spb >= 3.5 && spb <= (double)HD_CLOCKED_MAX_SPB)) return 0;
    return (uint32_t)(int64_t)std::floor(spb * 65536.0 + 0.5);
}

inline void clocked_state_reset(ClockedState& s, uint32_t F, uint32_t nbits, uint32_t nstops, uint32_t invert)
{
    std::memset(&s, 0, sizeof s);
    s.F = F; s.nbits = nbits; s.nstops = nstops; s.invert = invert;
    s.p = std::max<uint32_t>(2u, (F + 65536u) >> 17);                // the cursor starts at h
}

// What a launch that appends n samples may look at: the running sums P_{p-h} .. P_n.  Between launches p + look > n, so these are at most look + h + n.
inline uint32_t clocked_window_words(const ClockedState& s, uint32_t n)
{
    const uint64_t F = s.F;
    const uint32_t h = std::max<uint32_t>(2u, (uint32_t)((F + 65536u) >> 17));
    return 2u * h + (uint32_t)(((1u + s.nbits + s.nstops) * F + 32768u) >> 16) + n;
}

inline int32_t clocked_quantise(float v, uint32_t invert)
{
    if (v != v) return 0;
    const int32_t q = (int32_t)(std::min(std::max(v, -4.0f), 4.0f) * 1024.0f);
    return invert ? -q : q;
}

// One stream of the decoder: the state, the ring of running sums and the ring of records, as the kernel keeps them.
struct ClockedStream {
    ClockedState s{};
    std::vector<uint32_t> ring;
    std::vector<hd_clocked_record> rec;

    explicit ClockedStream(uint32_t record_cap) : ring(HD_CLOCKED_RING, 0u), rec(record_cap) { clocked_state_reset(s, 0, 0, 0, 0); }
    void reset() { set_modem(s.F, s.nbits, s.nstops, s.invert); }
    void set_modem(uint32_t F, uint32_t nbits, uint32_t nstops, uint32_t invert)
    {
        clocked_state_reset(s, F, nbits, nstops, invert);
        std::fill(ring.begin(), ring.end(), 0u);
    }
    uint32_t at(uint64_t i) const { return ring[(uint32_t)i & (HD_CLOCKED_RING - 1u)]; }
    int32_t S(uint64_t a, uint64_t b) const { return (int32_t)(at(b) - at(a)); }

    void push(const float* d, size_t n)
    {
        if (!s.F) return;
        for (size_t at0 = 0; at0 < n; at0 += HD_CLOCKED_CHUNK) {     // the ring holds one character's look-ahead and a chunk
            const size_t m = std::min<size_t>(HD_CLOCKED_CHUNK, n - at0);
            for (size_t j = 0; j < m; ++j) {
                s.total += (uint32_t)clocked_quantise(d[at0 + j], s.invert);
                s.n += 1;
                ring[(uint32_t)s.n & (HD_CLOCKED_RING - 1u)] = s.total;
            }
            scan();
        }
    }
    void scan()
    {
        const uint64_t F = s.F;
        const uint32_t nbits = s.nbits, K = 1u + nbits + s.nstops;
        const uint32_t full = (uint32_t)((F + 32768u) >> 16), h = std::max<uint32_t>(2u, (uint32_t)((F + 65536u) >> 17));
        const uint32_t look = h + (uint32_t)((K * F + 32768u) >> 16);
        auto B = [&](uint64_t x, uint32_t k) { return x + ((k * F + 32768u) >> 16); };
        while (s.p + look <= s.n) {
            const uint64_t p = s.p;
            if (!(S(p - h, p) > 0 && S(p, p + h) < 0)) { s.p += 1; continue; }
            uint64_t x = p;
            int32_t best = S(p, p + full) - S(p - h, p);
            for (uint64_t c = p + 1; c <= p + h; ++c) {
                const int32_t cost = S(c, c + full) - S(c - h, c);
                if (cost < best) { best = cost; x = c; }
            }
            const int32_t start = S(B(x, 0), B(x, 1)), stop = S(B(x, 1 + nbits), B(x, 2 + nbits));
            if (!(start < 0 && stop > 0)) { s.rejects += 1; s.p += 1; continue; }
            hd_clocked_record r;
            std::memset(&r, 0, sizeof r);
            r.pos = x; r.start = start; r.stop = stop;
            r.stop2 = s.nstops == 2 ? S(B(x, 2 + nbits), B(x, 3 + nbits)) : 0;
            for (uint32_t k = 0; k < nbits; ++k) {
                r.data[k] = S(B(x, 1 + k), B(x, 2 + k));
                r.ch |= (uint32_t)(r.data[k] > 0) << k;
            }
            if (s.written - s.taken >= rec.size()) { s.taken += 1; s.dropped += 1; }
            rec[s.written % rec.size()] = r;
            s.written += 1; s.chars += 1;
            s.p = x + (((2u * (1u + nbits) + 1u) * F + 65536u) >> 17);
        }
    }
    // up to cap of the oldest untaken records; out null: how many wait
    size_t take(hd_clocked_record* out, size_t cap)
    {
        const size_t have = (size_t)(s.written - s.taken);
        if (!out) return have;
        const size_t k = std::min(have, cap);
        for (size_t i = 0; i < k; ++i) out[i] = rec[(s.taken + i) % rec.size()];
        s.taken += k;
        return k;
    }
};

// The text stage behind the records: what TextStage::run does behind its framer, on characters that carry their records.
struct ClockedText {
    uint32_t repair_bits = 8, repair_flips = 3, nbits = 8;
    std::string text;
    std::vector<hd_clocked_record> recs;          // recs[i] is the record of text[i]
    std::deque<hd_clocked_sentence> out;
    uint64_t matches_failed = 0, plain = 0, repaired = 0;

    void reset() { text.clear(); recs.clear(); matches_failed = plain = repaired = 0; }
    void emit(const SentenceMatch& m, uint64_t pos, uint32_t flips)
    {
        const std::string t = m.callsign + "," + m.data + "*" + m.crc;
        hd_clocked_sentence s;
        std::memset(&s, 0, sizeof s);
        s.pos = pos; s.flips = flips; s.len = (uint32_t)t.size();
        std::memcpy(s.text, t.data(), std::min(t.size(), sizeof s.text - 1));
        out.push_back(s);
    }
    void feed(const hd_clocked_record* r, size_t n)
    {
        bool any = false;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t c = r[i].ch;
            if ((c >= 0x20 && c <= 0x7e) || c == '\n') { text.push_back((char)c); recs.push_back(r[i]); any = true; }
        }
        if (!any) return;
        SentenceMatch m;
        while (text.size() > 20 && extract_sentence(text, m)) {
            // the span in `text`: the scan leaves the CRC's last character in front of `rest`
            const size_t end = text.size() - m.rest.size() + 1, c0 = end - 5 - m.data.size() - 1 - m.callsign.size();
            size_t d0 = c0;
            while (d0 > 0 && text[d0 - 1] == '$') --d0;
            if (m.crc == crc16_ccitt_hex(m.callsign + "," + m.data)) {
                ++plain;
                emit(m, recs[d0].pos, 0);
            } else {
                ++matches_failed;
                std::vector<int32_t> data((end - d0) * 8);
                for (size_t i = d0; i < end; ++i) std::memcpy(&data[(i - d0) * 8], recs[i].data, sizeof recs[i].data);
                std::string fixed;
                SentenceMatch fm;
                const uint32_t flips = chase_repair(text.substr(d0, end - d0), data.data(), nbits, repair_bits, repair_flips, fixed, fm);
                if (flips) { ++repaired; emit(fm, recs[d0].pos, flips); }
            }
            recs.erase(recs.begin(), recs.begin() + (text.size() - m.rest.size()));
            text = m.rest;
        }
        if (text.size() > 1000) {
            const size_t cut = text.rfind('$');                      // (npos: erase(0, npos) empties the text, as the text stage's does)
            recs.erase(recs.begin(), cut == std::string::npos ? recs.end() : recs.begin() + cut);
            text.erase(0, cut);
        }
    }
    size_t take(hd_clocked_sentence* o, size_t cap)
    {
        size_t k = 0;
        for (; k < cap && !out.empty(); ++k) { o[k] = out.front(); out.pop_front(); }
        return k;
    }
};

}  // namespace hd
