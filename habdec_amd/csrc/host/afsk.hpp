// Host side of the AFSK / AX.25 modem (hd_afsk_*, include/habdec_amd.h has the definition): the parameters' checks, the flip patterns, the AX.25 encoder
// and the TNC2 formatter, the restatement of kernels/afsk.hip sample by sample and candidate by candidate, and the selection, delivery and counters that
// the engine's object runs too.  Plain C++, no GPU; exported as hd_host_afsk_* and hd_host_ax25_* (include/habdec_amd_host.h).  Not in the reference.
//
// Behind the quantisation everything is integer arithmetic: the kernels' slot and candidate records are held to this file byte for byte.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../../include/habdec_amd.h"
#include "afsk_state.hpp"
#include "clocked.hpp"
#include "tones.hpp"

namespace hd {

inline void afsk_params_default(hd_afsk_params* p)
{
    p->max_push = 0; p->max_frame_bytes = kAfskMaxFrame; p->repair_bits = 8; p->repair_flips = 2; p->require_addr = 1; p->_pad = 0;
}

// The flip patterns of repair_bits and repair_flips: the untouched one, then all subsets of size 1, 2, ... in lexicographic order.  False: more than 64.
inline bool afsk_patterns(uint32_t repair_bits, uint32_t repair_flips, uint32_t max_frame_bytes, AfskPatterns& t)
{
    std::memset(&t, 0, sizeof t);
    t.count = 1; t.max_frame_bytes = max_frame_bytes; t.L = afsk_walk_bits(max_frame_bytes);
    if (!repair_bits || !repair_flips) return true;
    if (repair_bits > 63u || repair_flips > kAfskMaxFlips) return false;
    t.list = repair_bits;
    for (uint32_t size = 1; size <= std::min(repair_flips, repair_bits); ++size) {
        uint32_t pos[kAfskMaxFlips];
        for (uint32_t i = 0; i < size; ++i) pos[i] = i;
        for (;;) {
            if (t.count == kAfskMaxPatterns) return false;
            uint64_t m = 0;
            for (uint32_t i = 0; i < size; ++i) m |= 1ull << pos[i];
            t.mask[t.count++] = m;
            int i = (int)size - 1;
            while (i >= 0 && pos[i] == repair_bits - size + (uint32_t)i) --i;
            if (i < 0) break;
            ++pos[i];
            for (uint32_t k = (uint32_t)i + 1; k < size; ++k) pos[k] = pos[k - 1] + 1u;
        }
    }
    return true;
}

// hd_afsk_create's checks: HD_OK with max_push filled in and the patterns made, or the error.
inline int afsk_params_check(hd_afsk_params& p, uint32_t default_push, AfskPatterns& t)
{
    if (p.max_frame_bytes < kAfskMinFrame || p.max_frame_bytes > kAfskMaxFrame || p.repair_flips > kAfskMaxFlips) return HD_ERR_INVALID;
    if (!afsk_patterns(p.repair_bits, p.repair_flips, p.max_frame_bytes, t)) return HD_ERR_INVALID;
    if (!p.max_push) p.max_push = default_push;
    if ((uint64_t)8u * t.L + kAfskBack + 8u + p.max_push > HD_AFSK_RING) return HD_ERR_UNSUPPORTED;
    return HD_OK;
}

inline void afsk_state_reset(AfskState& s, uint32_t F, uint32_t W, uint32_t mark, uint32_t space)
{
    std::memset(&s, 0, sizeof s);
    s.F = F; s.W = W; s.phi[0] = mark; s.phi[1] = space;
}
inline void afsk_state_reset(AfskState& s) { const AfskState was = s; afsk_state_reset(s, was.F, was.W, was.phi[0], was.phi[1]); }

// hd_afsk_set_modem's checks and the modem's integers: HD_OK and `s` reset with the modem, or the error and `s` untouched.
inline int afsk_modem(AfskState& s, double fsd, double baud, double mark, double space)
{
    if (!(fsd > 0) || !(baud > 0)) return HD_ERR_UNSUPPORTED;
    const double spb = fsd / baud;
    if (!(spb >= 8.0 && spb <= (double)HD_AFSK_MAX_SPB)) return HD_ERR_UNSUPPORTED;
    if (!(mark > 0 && mark < fsd / 2) || !(space > 0 && space < fsd / 2) || mark == space) return HD_ERR_INVALID;
    const double two32 = 4294967296.0;
    const uint64_t F = (uint64_t)(int64_t)std::floor(spb * 65536.0 + 0.5);
    afsk_state_reset(s, (uint32_t)F, (uint32_t)((F + 32768u) >> 16), (uint32_t)(int64_t)std::nearbyint(mark / fsd * two32),
                     (uint32_t)(int64_t)std::nearbyint(space / fsd * two32));
    return HD_OK;
}

inline uint32_t afsk_crc16(const uint8_t* p, size_t n)
{
    uint32_t crc = 0xFFFFu;
    for (size_t i = 0; i < n; ++i)
        for (uint32_t b = 0; b < 8; ++b) crc = afsk_crc_bit(crc, (p[i] >> b) & 1u);
    return crc ^ 0xFFFFu;
}

// ---- AX.25 UI frames

// "CALL" or "CALL-SSID" (a trailing '*' sets the H bit) -> the seven address bytes; false: no callsign of 1 .. 6 characters of 'A'-'Z', '0'-'9', or an
// SSID above 15.
inline bool ax25_address(const std::string& text, bool last, uint8_t* out)
{
    std::string t = text;
    bool h = false;
    if (!t.empty() && t.back() == '*') { h = true; t.pop_back(); }
    uint32_t ssid = 0;
    const size_t dash = t.find('-');
    if (dash != std::string::npos) {
        const std::string num = t.substr(dash + 1);
        if (num.empty() || num.size() > 2) return false;
        for (char c : num) { if (c < '0' || c > '9') return false; ssid = 10u * ssid + (uint32_t)(c - '0'); }
        if (ssid > 15u) return false;
        t.resize(dash);
    }
    if (t.empty() || t.size() > 6) return false;
    for (size_t i = 0; i < 6; ++i) {
        const char c = i < t.size() ? t[i] : ' ';
        if (!((c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || (c == ' ' && i >= t.size()))) return false;
        out[i] = (uint8_t)(c << 1);
    }
    out[6] = (uint8_t)(0x60u | (ssid << 1) | (last ? 1u : 0u) | (h ? 0x80u : 0u));
    return true;
}

// path: "SRC>DST" or "SRC>DST,DIGI1,DIGI2*" (the TNC2 order).  The frame's bytes with FCS; empty: a path that is none, or more than eight digipeaters.
inline std::vector<uint8_t> ax25_frame(const std::string& path, const uint8_t* info, size_t n_info)
{
    std::vector<std::string> part;
    const size_t gt = path.find('>');
    if (gt == std::string::npos) return {};
    const std::string src = path.substr(0, gt);
    size_t at = gt + 1;
    for (;;) {
        const size_t comma = path.find(',', at);
        part.push_back(path.substr(at, comma == std::string::npos ? std::string::npos : comma - at));
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    if (part.size() > 9) return {};
    std::vector<uint8_t> f(7 * (part.size() + 1));
    if (!ax25_address(part[0], false, f.data())) return {};
    if (!ax25_address(src, part.size() == 1, f.data() + 7)) return {};
    for (size_t k = 1; k < part.size(); ++k)
        if (!ax25_address(part[k], k + 1 == part.size(), f.data() + 7 * (k + 1))) return {};
    f.push_back(0x03); f.push_back(0xF0);
    f.insert(f.end(), info, info + n_info);
    const uint32_t crc = afsk_crc16(f.data(), f.size());
    f.push_back((uint8_t)(crc & 0xFFu)); f.push_back((uint8_t)(crc >> 8));
    return f;
}

// Frame bytes (FCS included) -> the NRZI level sequence: n_flags_before flags, the stuffed bits, n_flags_after flags, from the level `level` on.
inline std::vector<uint8_t> ax25_levels(const uint8_t* frame, size_t n, uint32_t flags_before, uint32_t flags_after, uint32_t level = 0)
{
    std::vector<uint8_t> bits;
    auto flag = [&] { for (uint32_t b = 0; b < 8; ++b) bits.push_back((0x7Eu >> b) & 1u); };
    for (uint32_t k = 0; k < flags_before; ++k) flag();
    uint32_t ones = 0;
    for (size_t i = 0; i < n; ++i)
        for (uint32_t b = 0; b < 8; ++b) {
            const uint8_t bit = (frame[i] >> b) & 1u;
            bits.push_back(bit);
            ones = bit ? ones + 1u : 0u;
            if (ones == 5u) { bits.push_back(0); ones = 0; }
        }
    for (uint32_t k = 0; k < flags_after; ++k) flag();
    std::vector<uint8_t> lv(bits.size());
    for (size_t i = 0; i < bits.size(); ++i) { if (!bits[i]) level ^= 1u; lv[i] = (uint8_t)level; }
    return lv;
}

// A UI frame without its FCS -> "SRC-SSID>DST,DIGI*:info".  HD_ERR_INVALID: an address field that fails the address check; HD_ERR_UNSUPPORTED: not UI.
inline int ax25_format(const uint8_t* d, size_t n, std::string& out)
{
    size_t end = 0;
    for (size_t i = 0; i < n && i < 70 && !end; ++i) {
        if (d[i] & 1u) { if (i % 7 == 6 && i >= 13) end = i; else return HD_ERR_INVALID; }
        else if (i % 7 < 6 && !afsk_callsign_byte(d[i])) return HD_ERR_INVALID;
    }
    if (!end) return HD_ERR_INVALID;
    const size_t m = (end + 1) / 7;
    if (n < end + 3 || d[end + 1] != 0x03 || d[end + 2] != 0xF0) return HD_ERR_UNSUPPORTED;
    auto call = [&](size_t k) {
        std::string s;
        for (size_t i = 0; i < 6; ++i) { const char c = (char)(d[7 * k + i] >> 1); if (c != ' ') s += c; }
        const uint32_t ssid = (d[7 * k + 6] >> 1) & 15u;
        if (ssid) s += "-" + std::to_string(ssid);
        return s;
    };
    size_t starred = 0;                                   // the last digipeater whose H bit is set
    for (size_t k = 2; k < m; ++k) if (d[7 * k + 6] & 0x80u) starred = k;
    out = call(1) + ">" + call(0);
    for (size_t k = 2; k < m; ++k) { out += "," + call(k); if (k == starred) out += "*"; }
    out += ":";
    for (size_t i = end + 3; i < n; ++i) {
        if (d[i] >= 32 && d[i] <= 126) out += (char)d[i];
        else { char buf[8]; std::snprintf(buf, sizeof buf, "<0x%02X>", d[i]); out += buf; }
    }
    return HD_OK;
}

// ---- one candidate

// The candidate at `slot`, a flag by the gate's rule; rec(g): d of slot g.  lv, conf: scratch of L + 1 entries.
template <typename Rec>
void afsk_decode(const AfskPatterns& t, uint32_t require_addr, uint64_t slot, Rec rec, std::vector<uint8_t>& lv, std::vector<uint32_t>& conf,
                 hd_afsk_candidate& o)
{
    const uint32_t L = t.L;
    lv.resize(L + 1u); conf.resize(L + 1u);
    for (uint32_t r = 0; r <= L; ++r) {
        const int32_t d = rec(slot + 8u * (uint64_t)r);
        lv[r] = d > 0;
        conf[r] = (uint32_t)(d < 0 ? -(int64_t)d : (int64_t)d);
    }
    std::memset(&o, 0, sizeof o);
    o.slot = slot;
    uint32_t flip[kAfskMaxFlips] = {~0u, ~0u, ~0u, ~0u};
    auto level = [&](uint32_t r) { return (uint32_t)lv[r] ^ (uint32_t)(r == flip[0] || r == flip[1] || r == flip[2] || r == flip[3]); };
    auto put = [&](uint32_t i, uint32_t b) { if (i < kAfskMaxFrame) o.data[i] = (uint8_t)b; };
    auto nothing = [](uint32_t, uint32_t) {};
    const AfskWalk hard = afsk_walk(level, L, t.max_frame_bytes, nothing);
    o.bits = hard.at;
    for (uint32_t r = 1; r <= hard.at; ++r) o.metric += conf[r];
    if (hard.kind != kAfskClose) { o.result = hard.kind == kAfskAbort ? HD_AFSK_ABORT : HD_AFSK_OPEN; return; }
    o.close_slot = slot + 8u * (uint64_t)hard.at;
    if (!hard.shaped) { o.result = HD_AFSK_UNSHAPED; return; }
    o.len = hard.bits >> 3;
    AfskWalk win = hard;
    if (hard.fcs_ok) o.result = hard.addr_ok || !require_addr ? HD_AFSK_PLAIN : HD_AFSK_REFUSED;
    else {
        o.result = HD_AFSK_FCS_FAILED;
        // the least confident levels of the bits 1 .. at - 8, ties to the earlier bit: keys (confidence, bit) in increasing order
        uint32_t list[64];
        uint32_t nl = 0;
        uint64_t last = 0;
        for (; nl < t.list; ++nl) {
            uint64_t best = ~0ull;
            for (uint32_t r = 1; r + 8u <= hard.at; ++r) {
                const uint64_t key = ((uint64_t)conf[r] << 12) | r;
                if ((!nl || key > last) && key < best) best = key;
            }
            if (best == ~0ull) break;
            list[nl] = (uint32_t)(best & 0xFFFu); last = best;
        }
        for (uint32_t j = 1; j < t.count; ++j) {
            uint32_t k = 0;
            bool fits = true;
            for (uint32_t b = 0; b < 64u; ++b)
                if ((t.mask[j] >> b) & 1u) { if (b >= nl) fits = false; else flip[k++] = list[b]; }
            for (uint32_t i = k; i < kAfskMaxFlips; ++i) flip[i] = ~0u;
            if (!fits) continue;
            const AfskWalk w = afsk_walk(level, hard.at, t.max_frame_bytes, nothing);
            if (w.kind != kAfskClose || w.at != hard.at || !w.shaped || !w.fcs_ok) continue;
            if (!w.addr_ok) { o.result = HD_AFSK_REFUSED; continue; }
            o.result = HD_AFSK_REPAIRED; o.flips = k; o.len = w.bits >> 3;
            win = w;
            break;
        }
        if (o.result != HD_AFSK_REPAIRED) for (uint32_t& f : flip) f = ~0u;
    }
    (void)afsk_walk(level, hard.at, t.max_frame_bytes, put);
    o.addr_ok = win.addr_ok; o.fcs = win.fcs;
}

// One stream of the modem.  The selection, the delivery and the counters serve the engine's object too (its kernels make the slots and the candidate
// records); the rings of the restatement exist only after host_rings().
struct AfskStream {
    AfskState s{};
    AfskPatterns pat{};
    uint32_t require_addr = 1;
    uint64_t decided = 0;                        // slots decided: every slot below it
    uint64_t flags = 0, unshaped = 0, fcs_failures = 0, frames_plain = 0, frames_repaired = 0, refused = 0, overlaps = 0;
    bool open = false;                           // a group's contest is open: its first candidate's slot, its best one so far
    uint64_t group_first = 0;
    uint64_t blocked_until = 0;                  // a passing candidate in front of it overlaps the frame delivered last: that frame's closing slot - 8
    hd_afsk_candidate best{};
    std::deque<hd_afsk_rx> waiting;
    std::deque<hd_afsk_candidate> log;           // every candidate, for hd_host_afsk_candidates and the test hook
    static constexpr size_t kLog = 16384;
    // the restatement's own
    std::vector<int32_t> C;
    std::vector<uint32_t> ring[4];
    std::vector<int32_t> slots;                  // [HD_AFSK_RING]
    std::vector<uint8_t> lv;
    std::vector<uint32_t> conf;

    AfskStream() { afsk_state_reset(s, 0, 0, 0, 0); }

    void host_rings()
    {
        C.resize(1024);
        tones_table(C.data());
        for (auto& r : ring) r.assign(kAfskRing32, 0u);
        slots.assign(HD_AFSK_RING, 0);
    }
    // (nothing behind index 0 is read: the rings need no clearing; frames not yet taken stay)
    void reset()
    {
        afsk_state_reset(s);
        decided = flags = unshaped = fcs_failures = frames_plain = frames_repaired = refused = overlaps = 0;
        open = false; blocked_until = 0;
        log.clear();
    }
    // The slots that can be decided once g slots exist: slot x's walk ends at slot x + 8 L at the latest.
    uint64_t decidable(uint64_t g) const
    {
        const uint64_t span = 8u * (uint64_t)pat.L;
        return s.F && g > span + decided ? g - span - decided : 0u;
    }

    // One candidate, in increasing slot order: counters, log, selection.
    void accept(const hd_afsk_candidate& o)
    {
        ++flags;
        if (log.size() == kLog) log.pop_front();
        log.push_back(o);
        switch (o.result) {
        case HD_AFSK_OPEN: case HD_AFSK_ABORT: case HD_AFSK_UNSHAPED: ++unshaped; return;
        case HD_AFSK_FCS_FAILED: ++fcs_failures; return;
        case HD_AFSK_REFUSED: ++refused; return;
        }
        if (o.slot < blocked_until) { ++overlaps; return; }
        if (open && o.slot < group_first + kAfskSettle) {
            if (o.flips < best.flips || (o.flips == best.flips && o.metric > best.metric)) best = o;
            return;
        }
        if (open) {
            deliver();
            if (o.slot < blocked_until) { ++overlaps; return; }
        }
        open = true; group_first = o.slot; best = o;
    }
    // n more slots are decided (the candidates among them have gone through accept): a group whose contest none of them can join any more delivers.
    void decided_more(uint64_t n)
    {
        decided += n;
        if (open && decided >= group_first + kAfskSettle) deliver();
    }
    void deliver()
    {
        hd_afsk_rx r;
        std::memset(&r, 0, sizeof r);
        r.slot = best.slot; r.start_sample = ((best.slot + 8u) * (uint64_t)s.F) >> 19; r.close_slot = best.close_slot; r.metric = best.metric;
        r.len = best.len - 2u; r.flips = best.flips; r.phase = (uint32_t)(best.slot & 7u); r.addr_ok = best.addr_ok; r.fcs = best.fcs;
        std::memcpy(r.data, best.data, r.len);
        waiting.push_back(r);
        ++(best.flips ? frames_repaired : frames_plain);
        open = false;
        blocked_until = best.close_slot > 8u ? best.close_slot - 8u : 0u;
    }
    size_t take(hd_afsk_rx* out, size_t cap)
    {
        if (!out) return waiting.size();
        size_t k = 0;
        for (; k < cap && !waiting.empty(); ++k) { out[k] = waiting.front(); waiting.pop_front(); }
        return k;
    }
    size_t take_log(hd_afsk_candidate* out, size_t cap)
    {
        if (!out) return log.size();
        size_t k = 0;
        for (; k < cap && !log.empty(); ++k) { out[k] = log.front(); log.pop_front(); }
        return k;
    }
    void stats(hd_afsk_counters* c, uint64_t samples, uint64_t slots_written) const
    {
        std::memset(c, 0, sizeof *c);
        c->samples = samples; c->slots = slots_written; c->flags = flags; c->unshaped = unshaped; c->fcs_failures = fcs_failures;
        c->frames_plain = frames_plain; c->frames_repaired = frames_repaired; c->refused = refused; c->overlaps = overlaps;
        c->F = s.F; c->W = s.W; c->step[0] = s.phi[0]; c->step[1] = s.phi[1];
    }

    // ---- the restatement: n samples make slots ...
    void push_samples(const float* row, size_t n)
    {
        if (!s.F) return;
        for (size_t j = 0; j < n; ++j) {
            const uint64_t i = s.n;
            const int32_t q = clocked_quantise(row[j], 0u);
            const bool slot = afsk_slot_end(s.F, s.g) == i;
            int64_t A[2] = {0, 0};
            for (uint32_t t = 0; t < 2; ++t) {
                const uint32_t a = ((uint32_t)i * s.phi[t]) >> 22;
                const int32_t r[2] = {(q * C[a]) >> 15, (-q * C[(a + 768u) & 1023u]) >> 15};
                int64_t w[2];
                for (uint32_t k = 0; k < 2; ++k) {
                    std::vector<uint32_t>& R = ring[2 * t + k];
                    const uint32_t now = s.tot[2 * t + k] + (uint32_t)r[k];
                    const uint32_t lag = i + 1 <= s.W ? 0u : R[(uint32_t)(i + 1 - s.W) & (kAfskRing32 - 1u)];      // read before the write below: W may be the ring's length
                    R[(uint32_t)(i + 1) & (kAfskRing32 - 1u)] = now;
                    s.tot[2 * t + k] = now;
                    w[k] = (int32_t)(now - lag);
                }
                if (slot) A[t] = (int64_t)tones_isqrt((uint64_t)(w[0] * w[0] + w[1] * w[1]));
            }
            if (slot) {
                slots[(size_t)(s.g & (HD_AFSK_RING - 1u))] = (int32_t)(A[0] - A[1]);
                ++s.g;
            }
            s.n = i + 1;
        }
    }
    int32_t slot_d(uint64_t g) const { return slots[(size_t)(g & (HD_AFSK_RING - 1u))]; }
    // the gate: slot g ends a flag on hard levels
    bool is_flag(uint64_t g) const
    {
        if (g < kAfskBack) return false;
        bool l[9];
        for (uint32_t j = 0; j < 9; ++j) l[j] = slot_d(g - 8u * (8u - j)) > 0;
        if (l[1] == l[0] || l[8] == l[7]) return false;
        for (uint32_t j = 2; j < 8; ++j) if (l[j] != l[1]) return false;
        return true;
    }
    // ... and every slot whose longest walk's last slot exists is decided
    void scan()
    {
        const uint64_t n = decidable(s.g);
        for (uint64_t k = 0; k < n; ++k) {
            if (!is_flag(decided + k)) continue;
            hd_afsk_candidate o;
            afsk_decode(pat, require_addr, decided + k, [this](uint64_t g) { return slot_d(g); }, lv, conf, o);
            accept(o);
        }
        decided_more(n);
    }
};

}  // namespace hd
