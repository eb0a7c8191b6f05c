// Host side of the Horus Binary 4FSK modem (hd_fsk4_*, include/habdec_amd.h has the definition): the frame descriptor's checks and tables, the encoder,
// the restatement of kernels/fsk4.hip sample by sample and candidate by candidate, and the selection, delivery and counters that the engine's object
// runs too.  Plain C++, no GPU; exported as hd_host_fsk4_* (include/habdec_amd_host.h).  Not in the reference.
//
// Behind the quantisation everything is integer arithmetic: the kernels' slot and candidate records are held to this file byte for byte.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <vector>

#include "../../../include/habdec_amd.h"
#include "fsk4_state.hpp"
#include "tones.hpp"

namespace hd {

inline void fsk4_params_default(hd_fsk4_params* p)
{
    p->max_push = 0; p->window_q8 = 256; p->uw_max_errors = 2; p->chase_bits = 4; p->max_corrected = -1; p->_pad = 0;
}
inline bool fsk4_window_ok(uint32_t window_q8) { return window_q8 >= 32 && window_q8 <= 256; }
inline bool fsk4_params_ok(const hd_fsk4_params* p) { return p->uw_max_errors <= 4 && p->chase_bits <= 6 && p->max_push <= (1u << 22); }

// Every format constant of the two presets: a correction is a change of one line here.
inline bool fsk4_preset(int preset, hd_fsk4_frame* f)
{
    switch (preset) {
    case HD_FSK4_HORUS_V1: *f = hd_fsk4_frame{22, {0x24, 0x24}, 0, 337, 0x4A80, 0xC75}; return true;
    case HD_FSK4_HORUS_V2: *f = hd_fsk4_frame{32, {0x24, 0x24}, 0, 503, 0x4A80, 0xC75}; return true;
    }
    return false;
}

inline uint32_t fsk4_codewords(uint32_t P) { return (8u * P + 11u) / 12u; }
inline uint32_t fsk4_body_bytes(uint32_t P) { return P + (11u * fsk4_codewords(P) + 7u) / 8u; }
inline uint32_t fsk4_symbols(uint32_t P) { return 4u * (2u + fsk4_body_bytes(P)); }

// A frame the decoder can take: its symbols fit the slot ring's reserve, the interleaver is a permutation, and the generator is one of the two of the
// (23,12) Golay code -- x^23 + 1 = (x + 1) g1 g2 over GF(2), so a divisor of degree 11 is g1 or g2.
inline bool fsk4_frame_ok(const hd_fsk4_frame& f)
{
    if (f.payload_bytes < 3 || f.payload_bytes > kFsk4MaxPayload) return false;
    const uint32_t bits = 8u * fsk4_body_bytes(f.payload_bytes);
    uint32_t a = f.interleave_mul, b = bits;
    if (!a || a >= bits) return false;
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    if (a != 1) return false;
    if (!f.scrambler_seed || f.scrambler_seed > 0x7FFFu) return false;
    if ((f.golay_poly >> 11) != 1u) return false;
    // x^23 + 1 modulo the generator: x^23 reduces like any bit above degree 10, the + 1 stays
    uint32_t r = 1u;                                     // x^0 ... multiply by x 23 times
    for (int k = 0; k < 23; ++k) { r <<= 1; if (r & 0x800u) r ^= f.golay_poly; }
    return (r ^ 1u) == 0u;
}

// The scrambler's first n outputs.
inline void fsk4_scrambler(uint32_t seed, uint8_t* out, uint32_t n)
{
    uint32_t state = seed;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t o = ((state >> 1) ^ state) & 1u;
        state = (state >> 1) | (o << 14);
        out[i] = (uint8_t)o;
    }
}

// Where body bit i (numbered least significant first, before the interleaver) is after it.
inline uint32_t fsk4_interleaved(const hd_fsk4_frame& f, uint32_t i) { return (uint32_t)(((uint64_t)f.interleave_mul * i) % (8u * fsk4_body_bytes(f.payload_bytes))); }

// The frame kernel's tables; false for a frame fsk4_frame_ok refuses (or a generator whose cosets do not all have a leader of weight <= 3: none passes
// fsk4_frame_ok, the table says so itself).
inline bool fsk4_tables(const hd_fsk4_frame& f, Fsk4Tab& t)
{
    if (!fsk4_frame_ok(f)) return false;
    std::memset(&t, 0, sizeof t);
    const uint32_t P = f.payload_bytes, K = fsk4_codewords(P), B = fsk4_body_bytes(P);
    t.nsym = fsk4_symbols(P); t.K = K; t.P = P; t.poly = f.golay_poly;
    t.uw = (uint32_t)f.uw[0] << 8 | f.uw[1];
    for (uint32_t& s : t.syn) s = 0xFFFFFFFFu;
    uint32_t filled = 0;
    auto put = [&](uint32_t e) { uint32_t& s = t.syn[fsk4_rem(e, f.golay_poly)]; if (s == 0xFFFFFFFFu) { s = e; ++filled; } };
    put(0);
    for (uint32_t a = 0; a < 23; ++a) {
        put(1u << a);
        for (uint32_t b = a + 1; b < 23; ++b) {
            put(1u << a | 1u << b);
            for (uint32_t c = b + 1; c < 23; ++c) put(1u << a | 1u << b | 1u << c);
        }
    }
    if (filled != 2048u) return false;
    std::vector<uint8_t> scr(8u * B);
    fsk4_scrambler(f.scrambler_seed, scr.data(), 8u * B);
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t b = 0; b < 23; ++b) {
            uint32_t i;                                  // the bit before the interleaver, numbered least significant first
            if (b < 12) {
                const uint32_t bit = 12u * k + b;        // of the payload, most significant first
                if (bit >= 8u * P) { t.src[23u * k + b] = kFsk4SrcPad; continue; }
                i = 8u * (bit / 8u) + 7u - bit % 8u;
            } else {
                const uint32_t q = 11u * k + (b - 12u);  // of the parity stream, most significant first
                i = 8u * (P + q / 8u) + 7u - q % 8u;
            }
            const uint32_t j = fsk4_interleaved(f, i);
            const uint32_t r = 16u + 8u * (j / 8u) + 7u - j % 8u;      // on the air, the unique word's 16 bits in front
            t.src[23u * k + b] = (uint16_t)(r | (scr[j] ? 0x8000u : 0u));
        }
    return true;
}

// payload (P bytes, the caller's CRC in the last two) -> the 2 + B bytes of the frame; returns their number, 0 for a frame fsk4_frame_ok refuses.
inline size_t fsk4_encode(const hd_fsk4_frame& f, const uint8_t* payload, uint8_t* out)
{
    if (!fsk4_frame_ok(f)) return 0;
    const uint32_t P = f.payload_bytes, K = fsk4_codewords(P), B = fsk4_body_bytes(P);
    std::vector<uint8_t> body(B, 0), mixed(B, 0), scr(8u * B);
    std::memcpy(body.data(), payload, P);
    for (uint32_t k = 0; k < K; ++k) {
        uint32_t data = 0;
        for (uint32_t b = 0; b < 12; ++b) {
            const uint32_t bit = 12u * k + b;
            data = data << 1 | (bit < 8u * P ? (payload[bit / 8u] >> (7u - bit % 8u)) & 1u : 0u);
        }
        const uint32_t parity = fsk4_rem(data << 11, f.golay_poly);
        for (uint32_t b = 0; b < 11; ++b) {
            const uint32_t q = 11u * k + b;
            body[P + q / 8u] |= (uint8_t)(((parity >> (10u - b)) & 1u) << (7u - q % 8u));
        }
    }
    fsk4_scrambler(f.scrambler_seed, scr.data(), 8u * B);
    for (uint32_t i = 0; i < 8u * B; ++i) {
        const uint32_t j = fsk4_interleaved(f, i);
        mixed[j / 8u] |= (uint8_t)(((body[i / 8u] >> (i % 8u)) & 1u) << (j % 8u));
    }
    for (uint32_t j = 0; j < 8u * B; ++j) mixed[j / 8u] ^= (uint8_t)(scr[j] << (j % 8u));
    out[0] = f.uw[0]; out[1] = f.uw[1];
    std::memcpy(out + 2, mixed.data(), B);
    return 2u + B;
}

inline uint32_t fsk4_crc16(const uint8_t* p, size_t n)
{
    uint32_t crc = 0xFFFFu;
    for (size_t i = 0; i < n; ++i) crc = fsk4_crc16_byte(crc, p[i]);
    return crc;
}

// The state a reset gives a stream with this modem (F = 0: none).
inline void fsk4_state_reset(Fsk4State& s, uint32_t F, uint32_t W, const uint32_t* phi)
{
    std::memset(&s, 0, sizeof s);
    s.F = F; s.W = W;
    for (uint32_t t = 0; t < 4; ++t) s.phi[t] = phi ? phi[t] : 0u;
}
inline void fsk4_state_reset(Fsk4State& s) { const Fsk4State was = s; fsk4_state_reset(s, was.F, was.W, was.phi); }

// hd_fsk4_set_modem's checks of the clock and the tones, and the modem's integers: HD_OK and `s` reset with the modem, or the error and `s` untouched.
inline int fsk4_modem(Fsk4State& s, double fsd, double baud, double f0, double spacing, uint32_t window_q8)
{
    if (!(fsd > 0) || !(baud > 0) || !fsk4_window_ok(window_q8)) return HD_ERR_UNSUPPORTED;
    const double spb = fsd / baud;
    if (!(spb >= 8.0 && spb <= (double)HD_FSK4_MAX_SPB)) return HD_ERR_UNSUPPORTED;
    uint32_t phi[4];
    const double two32 = 4294967296.0;
    for (uint32_t t = 0; t < 4; ++t) {
        const double f = f0 + t * spacing;
        if (!(std::fabs(f) < fsd / 2)) return HD_ERR_INVALID;
        phi[t] = (uint32_t)(int64_t)std::nearbyint(f / fsd * two32);
    }
    const uint64_t F = (uint64_t)(int64_t)std::floor(spb * 65536.0 + 0.5);
    const uint64_t W = std::max<uint64_t>(1u, (F * window_q8 + (1u << 23)) >> 24);
    fsk4_state_reset(s, (uint32_t)F, (uint32_t)W, phi);
    return HD_OK;
}

// hd_fsk4_retune's checks and the new tones' steps, by set_modem's rule: HD_ERR_INVALID for a tone outside +- fsd / 2 (or a non-finite one).
inline int fsk4_retune_steps(double fsd, double f0, double spacing, uint32_t* phi)
{
    for (uint32_t t = 0; t < 4; ++t) {
        const double f = f0 + t * spacing;
        if (!(std::fabs(f) < fsd / 2)) return HD_ERR_INVALID;
        phi[t] = (uint32_t)(int64_t)std::nearbyint(f / fsd * 4294967296.0);
    }
    return HD_OK;
}
// A retune that waits for its sample.
struct Fsk4Retune {
    uint64_t at;
    uint32_t phi[4];
};

// Slots a stream's ring holds, a power of two: the 8 (260 - 1) slots a candidate may wait for its last one, a push's new slots (at most one per sample,
// at 8 samples per symbol) and the slot in flight.
inline uint32_t fsk4_slot_cap(uint32_t max_push)
{
    const uint32_t need = 8u * (kFsk4MaxSymbols + (max_push + 7u) / 8u + 1u);
    uint32_t cap = 4096;
    while (cap < need) cap <<= 1;
    return cap;
}

// Steps 1 .. 6 of the definition for the candidate at `slot`; rec(g): the four envelopes of slot g.  False: the unique-word gate refused it.
template <typename Rec>
bool fsk4_decode(const Fsk4Tab& t, uint32_t uw_max_errors, uint32_t chase_bits, uint64_t slot, Rec rec, Fsk4Out& o)
{
    int32_t soft[2 * kFsk4MaxSymbols];
    uint32_t uw_err = 0;
    uint64_t metric = 0;
    for (uint32_t m = 0; m < t.nsym; ++m) {
        const uint32_t* E = rec(slot + 8u * m);
        uint32_t best = 0;
        for (uint32_t v = 1; v < 4; ++v) if (E[v] > E[best]) best = v;
        if (m < 8) uw_err += (uint32_t)__builtin_popcount(best ^ ((t.uw >> (14u - 2u * m)) & 3u));
        metric += E[best];
        soft[2 * m] = (int32_t)std::max(E[2], E[3]) - (int32_t)std::max(E[0], E[1]);
        soft[2 * m + 1] = (int32_t)std::max(E[1], E[3]) - (int32_t)std::max(E[0], E[2]);
    }
    if (uw_err > uw_max_errors) return false;
    std::memset(&o, 0, sizeof o);
    o.slot = slot; o.metric = metric; o.uw_errors = uw_err;
    uint32_t data[kFsk4MaxCodewords];
    for (uint32_t k = 0; k < t.K; ++k) {
        uint32_t conf[23], h = 0;
        for (uint32_t b = 0; b < 23; ++b) {
            const uint16_t e = t.src[23u * k + b];
            const int32_t v = e == kFsk4SrcPad ? -kFsk4PadConfidence : (e & 0x8000u) ? -soft[e & 0x3FFu] : soft[e & 0x3FFu];
            conf[b] = (uint32_t)(v < 0 ? -v : v);
            h |= (uint32_t)(v > 0) << (22u - b);
        }
        uint32_t lc[6], taken = 0;
        for (uint32_t c = 0; c < chase_bits; ++c) {
            uint32_t pick = 23;
            for (uint32_t b = 0; b < 23; ++b)
                if (!((taken >> b) & 1u) && (pick == 23 || conf[b] < conf[pick])) pick = b;
            lc[c] = pick; taken |= 1u << pick;
        }
        uint64_t best_key = ~0ull;
        uint32_t best_cw = 0;
        for (uint32_t pn = 0; pn < (1u << chase_bits); ++pn) {
            uint32_t w = h;
            for (uint32_t c = 0; c < chase_bits; ++c) if ((pn >> c) & 1u) w ^= 1u << (22u - lc[c]);
            const uint32_t cw = w ^ t.syn[fsk4_rem(w, t.poly)];
            uint64_t cost = 0;
            for (uint32_t d = cw ^ h, b = 0; b < 23; ++b) if ((d >> (22u - b)) & 1u) cost += conf[b];
            const uint64_t key = cost << 6 | pn;
            if (key < best_key) { best_key = key; best_cw = cw; }
        }
        o.corrected += (uint32_t)__builtin_popcount(best_cw ^ h);
        data[k] = best_cw >> 11;
    }
    for (uint32_t b = 0; b < t.P; ++b) {
        uint32_t byte = 0;
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t bit = 8u * b + i;
            byte = byte << 1 | ((data[bit / 12u] >> (11u - bit % 12u)) & 1u);
        }
        o.payload[b] = (uint8_t)byte;
    }
    o.crc_ok = fsk4_crc16(o.payload, t.P - 2u) == ((uint32_t)o.payload[t.P - 2u] | (uint32_t)o.payload[t.P - 1u] << 8);
    return true;
}

// One stream of the modem.  The tables, the selection, the delivery and the counters serve the engine's object too (its kernels make the slots and the
// candidate records); rings and table of the restatement exist only after host_rings().
struct Fsk4Stream {
    Fsk4State s{};
    Fsk4Tab tab{};
    uint32_t uw_max_errors = 2, chase_bits = 4;
    int32_t max_corrected = -1;
    uint64_t decided = 0;                        // candidates decided: every slot below it
    uint64_t candidates = 0, gate_passes = 0, crc_failures = 0, refused = 0, overlaps = 0, frames = 0;
    bool open = false;                           // a group's contest is open: its first candidate's slot, its best one so far
    uint64_t group_first = 0;
    uint64_t blocked_until = 0;                  // a candidate in front of it overlaps the frame delivered last: that frame's slot + 8 (symbols - 1)
    Fsk4Out best{};
    std::deque<hd_fsk4_rx> waiting;
    std::deque<hd_fsk4_candidate> log;           // the candidates behind the gate, for hd_host_fsk4_candidates and the test hook
    static constexpr size_t kLog = 65536;
    std::deque<Fsk4Retune> pending;              // retunes that wait for their sample, in the order of the calls
    uint64_t retunes = 0, late = 0;              // retunes that took effect; those of them whose sample was behind the stream's index
    // the restatement's own
    std::vector<int32_t> C;
    std::vector<uint32_t> ring[8];
    std::vector<uint32_t> slots;                 // [slot_cap][4]
    uint32_t slot_cap = 0;

    Fsk4Stream() { fsk4_state_reset(s, 0, 0, nullptr); }

    void set_params(const hd_fsk4_params& p) { uw_max_errors = p.uw_max_errors; chase_bits = p.chase_bits; max_corrected = p.max_corrected; }
    void host_rings(uint32_t max_push)
    {
        C.resize(1024);
        tones_table(C.data());
        for (auto& r : ring) r.assign(kFsk4Ring32, 0u);
        slot_cap = fsk4_slot_cap(max_push);
        slots.assign((size_t)slot_cap * 4u, 0u);
    }
    // (nothing behind index 0 is read: the rings need no clearing; frames not yet taken stay)
    void reset()
    {
        fsk4_state_reset(s);
        decided = candidates = gate_passes = crc_failures = refused = overlaps = frames = 0;
        open = false; blocked_until = 0;
        log.clear();
        pending.clear();
        retunes = late = 0;
    }
    // hd_fsk4_retune.  The retunes take effect in the order of the calls: the one in front waits for its sample, those behind it for the one in front.
    void retune(const uint32_t* phi, uint64_t at)
    {
        Fsk4Retune r;
        r.at = at;
        for (uint32_t t = 0; t < 4; ++t) r.phi[t] = phi[t];
        pending.push_back(r);
    }
    // In front of sample s.n: every retune in front of the queue whose sample is s.n or behind it takes effect at s.n, Psi_t += s.n (Phi_old - Phi_new)
    // mod 2^32 -- the rotator's phase at s.n is what it would have been.  True: the state changed (the engine's object copies phi and psi to the device).
    bool apply_retunes()
    {
        bool any = false;
        for (; !pending.empty() && pending.front().at <= s.n; pending.pop_front()) {
            const Fsk4Retune& r = pending.front();
            for (uint32_t t = 0; t < 4; ++t) {
                s.psi[t] += (uint32_t)s.n * (s.phi[t] - r.phi[t]);
                s.phi[t] = r.phi[t];
            }
            ++retunes;
            late += r.at < s.n;
            any = true;
        }
        return any;
    }
    // Samples from s.n on that no waiting retune cuts (after apply_retunes()): at most `want`.
    uint64_t uncut(uint64_t want) const { return pending.empty() ? want : std::min<uint64_t>(want, pending.front().at - s.n); }
    uint32_t limit() const { return max_corrected < 0 ? 2u * tab.K : (uint32_t)max_corrected; }

    // The candidates that can be decided once g slots exist, first and count: a candidate's last slot is its first + 8 (nsym - 1).
    uint64_t decidable(uint64_t g) const
    {
        const uint64_t span = 8u * (uint64_t)(tab.nsym - 1u);
        return s.F && tab.nsym && g > span + decided ? g - span - decided : 0u;
    }

    // One candidate behind the gate, in increasing slot order: counters, log, selection.
    void accept(const Fsk4Out& o)
    {
        ++gate_passes;
        hd_fsk4_candidate c;
        std::memset(&c, 0, sizeof c);
        c.slot = o.slot; c.metric = o.metric; c.crc_ok = o.crc_ok; c.corrected = o.corrected; c.uw_errors = o.uw_errors;
        std::memcpy(c.payload, o.payload, sizeof c.payload);
        if (log.size() == kLog) log.pop_front();
        log.push_back(c);
        if (!o.crc_ok) { ++crc_failures; return; }
        if (o.corrected > limit()) { ++refused; return; }
        if (o.slot < blocked_until) { ++overlaps; return; }
        if (open && o.slot < group_first + kFsk4Settle) {
            if (o.corrected < best.corrected || (o.corrected == best.corrected && o.metric > best.metric)) best = o;
            return;
        }
        if (open) {
            deliver();
            if (o.slot < blocked_until) { ++overlaps; return; }
        }
        open = true; group_first = o.slot; best = o;
    }
    // n more candidates are decided (those behind the gate have gone through accept): a group whose contest none of them can join any more delivers.
    void decided_more(uint64_t n)
    {
        candidates += n; decided += n;
        if (open && decided >= group_first + kFsk4Settle) deliver();
    }
    void deliver()
    {
        hd_fsk4_rx r;
        std::memset(&r, 0, sizeof r);
        r.slot = best.slot; r.start_sample = (best.slot * (uint64_t)s.F) >> 19; r.metric = best.metric;
        r.payload_bytes = tab.P; r.corrected = best.corrected; r.phase = (uint32_t)(best.slot & 7u); r.uw_errors = best.uw_errors;
        std::memcpy(r.payload, best.payload, sizeof r.payload);
        waiting.push_back(r);
        ++frames;
        open = false;
        blocked_until = best.slot + 8u * (uint64_t)(tab.nsym - 1u);
    }
    size_t take(hd_fsk4_rx* out, size_t cap)
    {
        if (!out) return waiting.size();
        size_t k = 0;
        for (; k < cap && !waiting.empty(); ++k) { out[k] = waiting.front(); waiting.pop_front(); }
        return k;
    }
    size_t take_log(hd_fsk4_candidate* out, size_t cap)
    {
        if (!out) return log.size();
        size_t k = 0;
        for (; k < cap && !log.empty(); ++k) { out[k] = log.front(); log.pop_front(); }
        return k;
    }
    void stats(hd_fsk4_counters* c, uint64_t samples, uint64_t slots_written) const
    {
        std::memset(c, 0, sizeof *c);
        c->samples = samples; c->slots = slots_written; c->candidates = candidates; c->gate_passes = gate_passes; c->crc_failures = crc_failures;
        c->refused = refused; c->overlaps = overlaps; c->frames = frames;
        c->F = s.F; c->W = s.W;
        for (uint32_t t = 0; t < 4; ++t) c->step[t] = s.phi[t];
        c->symbols = s.F ? tab.nsym : 0u; c->codewords = s.F ? tab.K : 0u;
    }

    // ---- the restatement: n cf32 samples at iq (re, im interleaved) make slots ...
    void push_samples(const float* iq, size_t n)
    {
        if (!s.F) return;
        for (size_t j = 0; j < n; ++j) {
            const uint64_t i = s.n;
            if (!pending.empty()) apply_retunes();
            const int32_t q_re = tones_quantise(iq[2 * j]), q_im = tones_quantise(iq[2 * j + 1]);
            const bool slot = fsk4_slot_end(s.F, s.g) == i;
            uint32_t A[4];
            for (uint32_t t = 0; t < 4; ++t) {
                const uint32_t a = ((uint32_t)i * s.phi[t] + s.psi[t]) >> 22;
                const int32_t c = C[a], sn = C[(a + 768u) & 1023u];
                const int32_t r[2] = {(q_re * c + q_im * sn) >> 15, (q_im * c - q_re * sn) >> 15};
                int64_t w[2];
                for (uint32_t k = 0; k < 2; ++k) {
                    std::vector<uint32_t>& R = ring[2 * t + k];
                    const uint32_t now = s.tot[2 * t + k] + (uint32_t)r[k];
                    const uint32_t lag = i + 1 <= s.W ? 0u : R[(uint32_t)(i + 1 - s.W) & (kFsk4Ring32 - 1u)];      // read before the write below: W may be the ring's length
                    R[(uint32_t)(i + 1) & (kFsk4Ring32 - 1u)] = now;
                    s.tot[2 * t + k] = now;
                    w[k] = (int32_t)(now - lag);
                }
                A[t] = slot ? tones_isqrt((uint64_t)(w[0] * w[0] + w[1] * w[1])) : 0u;
            }
            if (slot) {
                std::memcpy(&slots[(size_t)(s.g & (slot_cap - 1u)) * 4u], A, sizeof A);
                ++s.g;
            }
            s.n = i + 1;
        }
    }
    // ... and every candidate whose last slot exists is decided
    void scan()
    {
        const uint64_t n = decidable(s.g);
        for (uint64_t k = 0; k < n; ++k) {
            Fsk4Out o;
            if (fsk4_decode(tab, uw_max_errors, chase_bits, decided + k, [this](uint64_t g) { return &slots[(size_t)(g & (slot_cap - 1u)) * 4u]; }, o)) accept(o);
        }
        decided_more(n);
    }
};

}  // namespace hd
