// Host side of the SSDV packet receiver (hd_ssdv_*, include/habdec_amd.h has the definition): the field, an encoder, the decoder with its four trials,
// CRC-32, the header, the gap rule and the greedy delivery.  Plain C++, no GPU; exported as hd_host_ssdv_* (include/habdec_amd_host.h).  The stream
// bookkeeping (SsdvStream: the doors, the gap rule, the delivery, the counters) is the code the engine's object runs; the decoder (ssdv_decode) restates
// kernels/ssdv.hip by another route -- log / antilog tables, Berlekamp-Massey with an inverse, Forney -- and the kernel is held to its outcomes byte for
// byte.  Not in the reference.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <deque>
#include <vector>

#include "../../../include/habdec_amd.h"

namespace hd {

constexpr uint32_t kSsdvPoly = 0x187u, kSsdvRoots = 32u, kSsdvFcr = 112u, kSsdvPrim = 11u, kSsdvData = 223u, kSsdvCrcLen = 219u;
constexpr uint32_t kSsdvTrials = 4u, kSsdvMaxErasures = 24u;
constexpr uint32_t kSsdvConfMax = 0xFFFFFFu;

// GF(2^8) modulo x^8 + x^7 + x^2 + x + 1, alpha = 2.  root[m] = alpha^(11 (112 + m)); loc[j] = beta^(255 - j) with beta = alpha^11: the locator of byte j.
struct SsdvField {
    uint8_t exp[512], log[256], root[kSsdvRoots], loc[256], gen[kSsdvRoots + 1];     // gen[k]: the generator's coefficient of x^k
    SsdvField()
    {
        uint32_t v = 1;
        for (uint32_t i = 0; i < 255; ++i) {
            exp[i] = exp[i + 255] = (uint8_t)v; log[v] = (uint8_t)i;
            v <<= 1;
            if (v & 0x100u) v ^= kSsdvPoly;
        }
        exp[510] = exp[0]; exp[511] = exp[1]; log[0] = 0;
        for (uint32_t m = 0; m < kSsdvRoots; ++m) root[m] = exp[(kSsdvPrim * (kSsdvFcr + m)) % 255u];
        for (uint32_t j = 0; j < 256; ++j) loc[j] = exp[(kSsdvPrim * ((255u - j) % 255u)) % 255u];
        std::memset(gen, 0, sizeof gen);
        gen[0] = 1;
        for (uint32_t m = 0; m < kSsdvRoots; ++m) {                  // gen *= (x + root[m])
            for (uint32_t k = m + 1; k > 0; --k) gen[k] = (uint8_t)(gen[k - 1] ^ mul(gen[k], root[m]));
            gen[0] = mul(gen[0], root[m]);
        }
    }
    uint8_t mul(uint8_t a, uint8_t b) const { return a && b ? exp[log[a] + log[b]] : 0; }
    uint8_t inv(uint8_t a) const { return exp[255 - log[a]]; }       // a != 0
};
inline const SsdvField& ssdv_field() { static const SsdvField f; return f; }

// parity[0] is byte 224 of the packet (the coefficient of x^31), parity[31] byte 255
inline void ssdv_encode(const uint8_t* data223, uint8_t* parity32)
{
    const SsdvField& F = ssdv_field();
    uint8_t bb[kSsdvRoots] = {0};
    for (uint32_t i = 0; i < kSsdvData; ++i) {
        const uint8_t fb = (uint8_t)(data223[i] ^ bb[0]);
        for (uint32_t k = 0; k + 1 < kSsdvRoots; ++k) bb[k] = (uint8_t)(bb[k + 1] ^ F.mul(fb, F.gen[kSsdvRoots - 1 - k]));
        bb[kSsdvRoots - 1] = F.mul(fb, F.gen[0]);
    }
    std::memcpy(parity32, bb, kSsdvRoots);
}

inline uint32_t ssdv_crc32(const uint8_t* p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}
// pkt: the 256 bytes, byte 0 the sync byte
inline bool ssdv_crc_ok(const uint8_t* pkt)
{
    const uint32_t c = ssdv_crc32(pkt + 1, kSsdvCrcLen);
    return pkt[220] == (uint8_t)(c >> 24) && pkt[221] == (uint8_t)(c >> 16) && pkt[222] == (uint8_t)(c >> 8) && pkt[223] == (uint8_t)c;
}

// The first six characters count (40^6 < 2^32: no wrap); a character outside A-Z, a-z and 0-9 becomes digit 0, which reads back as '-'.
inline uint32_t ssdv_callsign_code(const char* s)
{
    uint32_t x = 0;
    for (size_t k = s ? std::min<size_t>(std::strlen(s), 6) : 0; k > 0; --k) {
        const char ch = s[k - 1];
        x *= 40u;
        if (ch >= 'A' && ch <= 'Z') x += (uint32_t)(ch - 'A') + 14u;
        else if (ch >= 'a' && ch <= 'z') x += (uint32_t)(ch - 'a') + 14u;
        else if (ch >= '0' && ch <= '9') x += (uint32_t)(ch - '0') + 1u;
    }
    return x;
}

// The header fields of p->data into p (after the CRC no field is tested for plausibility).
inline void ssdv_header(hd_ssdv_packet* p)
{
    const uint8_t* d = p->data;
    p->type = d[1];
    uint32_t code = (uint32_t)d[2] << 24 | (uint32_t)d[3] << 16 | (uint32_t)d[4] << 8 | d[5];
    std::memset(p->callsign, 0, sizeof p->callsign);
    for (uint32_t k = 0; code && k + 1 < sizeof p->callsign; ++k, code /= 40u) {
        const uint32_t s = code % 40u;
        p->callsign[k] = s == 0 ? '-' : s < 11 ? (char)('0' + s - 1) : s < 14 ? '-' : (char)('A' + s - 14);
    }
    p->image_id = d[6];
    p->packet_id = (uint32_t)d[7] << 8 | d[8];
    p->width = (uint32_t)d[9] * 16u; p->height = (uint32_t)d[10] * 16u;
    p->flags = d[11]; p->mcu_offset = d[12];
    p->mcu_index = (uint32_t)d[13] << 8 | d[14];
}

// A whole packet: sync, the 14 header bytes, 205 payload bytes, CRC-32, parity.  A packet of type HD_SSDV_TYPE_NOFEC (0x67) carries zeros where the
// parity would be: only its CRC protects it.
inline void ssdv_make_packet(uint8_t type, const char* callsign, uint8_t image_id, uint16_t packet_id, uint16_t width, uint16_t height, uint8_t flags,
                             uint8_t mcu_offset, uint16_t mcu_index, const uint8_t* payload205, uint8_t* out256)
{
    uint8_t* d = out256;
    const uint32_t code = ssdv_callsign_code(callsign);
    d[0] = 0x55; d[1] = type;
    d[2] = (uint8_t)(code >> 24); d[3] = (uint8_t)(code >> 16); d[4] = (uint8_t)(code >> 8); d[5] = (uint8_t)code;
    d[6] = image_id; d[7] = (uint8_t)(packet_id >> 8); d[8] = (uint8_t)packet_id;
    d[9] = (uint8_t)(width / 16u); d[10] = (uint8_t)(height / 16u); d[11] = flags; d[12] = mcu_offset;
    d[13] = (uint8_t)(mcu_index >> 8); d[14] = (uint8_t)mcu_index;
    std::memcpy(d + 15, payload205, 205);
    const uint32_t c = ssdv_crc32(d + 1, kSsdvCrcLen);
    d[220] = (uint8_t)(c >> 24); d[221] = (uint8_t)(c >> 16); d[222] = (uint8_t)(c >> 8); d[223] = (uint8_t)c;
    if (type == HD_SSDV_TYPE_NOFEC) std::memset(d + 224, 0, kSsdvRoots);
    else ssdv_encode(d + 1, d + 224);
}

// syn[m] = the word's polynomial at root[m]; r[1 .. 255] is the word.  Returns whether all are zero.
inline bool ssdv_syndromes(const uint8_t* r, uint8_t* syn)
{
    const SsdvField& F = ssdv_field();
    uint8_t any = 0;
    for (uint32_t m = 0; m < kSsdvRoots; ++m) {
        uint8_t s = 0;
        for (uint32_t j = 1; j <= 255; ++j) s = (uint8_t)(F.mul(s, F.root[m]) ^ r[j]);
        syn[m] = s; any |= s;
    }
    return !any;
}

// One trial: the codeword w (w[1 .. 255]) with 2 e + f <= 32 around r, f erasures at era[0 .. f), if there is one.
inline bool ssdv_trial(const uint8_t* r, const uint8_t* syn, const uint8_t* era, uint32_t f, uint8_t* w, uint32_t* errors, uint32_t* changed)
{
    const SsdvField& F = ssdv_field();
    constexpr uint32_t R = kSsdvRoots;
    uint8_t lam[R + 1] = {0}, b[R + 1], t[R + 1];
    lam[0] = 1;
    for (uint32_t i = 0; i < f; ++i) {
        const uint8_t X = F.loc[era[i]];
        for (uint32_t k = i + 1; k > 0; --k) lam[k] ^= F.mul(X, lam[k - 1]);
    }
    std::memcpy(b, lam, sizeof b);
    uint32_t el = f;
    for (uint32_t rr = f + 1; rr <= R; ++rr) {
        uint8_t d = 0;
        for (uint32_t i = 0; i < rr; ++i) d ^= F.mul(lam[i], syn[rr - 1 - i]);
        if (!d) {
            std::memmove(b + 1, b, R); b[0] = 0;
            continue;
        }
        t[0] = lam[0];
        for (uint32_t i = 0; i < R; ++i) t[i + 1] = (uint8_t)(lam[i + 1] ^ F.mul(d, b[i]));
        if (2 * el <= rr + f - 1) {
            el = rr + f - el;
            const uint8_t di = F.inv(d);
            for (uint32_t i = 0; i <= R; ++i) b[i] = F.mul(lam[i], di);
        } else {
            std::memmove(b + 1, b, R); b[0] = 0;
        }
        std::memcpy(lam, t, sizeof lam);
    }
    uint32_t deg = 0;
    for (uint32_t i = 0; i <= R; ++i) if (lam[i]) deg = i;
    if (deg < f || 2 * (deg - f) + f > R) return false;
    // the roots: byte j is in error iff lam(1 / loc[j]) == 0, and 1 / loc[j] = loc[255 - j]
    uint8_t at[R];
    uint32_t count = 0;
    for (uint32_t j = 1; j <= 255; ++j) {
        const uint8_t xi = F.loc[255 - j];
        uint8_t v = 0;
        for (uint32_t k = deg + 1; k > 0; --k) v = (uint8_t)(F.mul(v, xi) ^ lam[k - 1]);
        if (!v) { if (count < R) at[count] = (uint8_t)j; ++count; }
    }
    if (count != deg) return false;
    uint8_t om[R];
    for (uint32_t i = 0; i < R; ++i) {
        uint8_t v = 0;
        for (uint32_t k = 0; k <= std::min(i, deg); ++k) v ^= F.mul(lam[k], syn[i - k]);
        om[i] = v;
    }
    std::memcpy(w, r, 256);
    for (uint32_t q = 0; q < count; ++q) {
        const uint32_t j = at[q];
        const uint8_t xi = F.loc[255 - j];
        uint8_t num = 0, den = 0, p2 = 1;
        const uint8_t x2 = F.mul(xi, xi);
        for (uint32_t k = R; k > 0; --k) num = (uint8_t)(F.mul(num, xi) ^ om[k - 1]);
        for (uint32_t k = 1; k <= R; k += 2) { den ^= F.mul(lam[k], p2); p2 = F.mul(p2, x2); }     // the formal derivative: the odd coefficients
        if (!den) return false;
        // the error value: X^(1 - fcr) * omega(1 / X) / lambda'(1 / X), X = loc[j]; X^(1 - fcr) = (1 / X)^(fcr - 1)
        const uint8_t xp = F.exp[(F.log[xi] * (kSsdvFcr - 1u)) % 255u];
        w[j] ^= F.mul(F.mul(num, xp), F.inv(den));
    }
    uint8_t s2[R];
    if (!ssdv_syndromes(w, s2)) return false;
    bool erased[256] = {false};
    for (uint32_t i = 0; i < f; ++i) erased[era[i]] = true;
    uint32_t e = 0, ch = 0;
    for (uint32_t j = 1; j <= 255; ++j) if (w[j] != r[j]) { if (erased[j]) ++ch; else ++e; }
    if (2 * e + f > R) return false;
    *errors = e; *changed = ch;
    return true;
}

// The candidate whose byte 0 is word[0]: word[k] = (c << 8) | b of byte k, 256 of them.  True: out holds the packet (pos is the caller's); crc_bad grows
// by the trials that found a codeword whose CRC is wrong.
inline bool ssdv_decode(const uint32_t* word, hd_ssdv_packet* out, uint64_t* crc_bad)
{
    uint8_t r[256], w[256], syn[kSsdvRoots], era[kSsdvMaxErasures];
    for (uint32_t k = 0; k < 256; ++k) r[k] = (uint8_t)word[k];
    auto accept = [&](const uint8_t* pkt, uint32_t trial, uint32_t e, uint32_t f, uint32_t ch) {
        std::memset(out, 0, sizeof *out);
        out->trial = trial; out->errors = e; out->erasures = f; out->erasures_changed = ch;
        std::memcpy(out->data, pkt, 256);
        out->data[0] = 0x55;
        ssdv_header(out);
        return true;
    };
    if (r[0] == 0x55 && r[1] == HD_SSDV_TYPE_NOFEC && ssdv_crc_ok(r)) return accept(r, HD_SSDV_NOFEC, 0, 0, 0);
    const bool clean = ssdv_syndromes(r, syn);
    if (clean) {                                                     // every trial finds r itself
        if (ssdv_crc_ok(r)) return accept(r, 0, 0, 0, 0);
        *crc_bad += kSsdvTrials;
        return false;
    }
    uint32_t key[255];
    for (uint32_t j = 1; j <= 255; ++j) key[j - 1] = (word[j] & ~0xFFu) | j;
    std::partial_sort(key, key + kSsdvMaxErasures, key + 255);
    for (uint32_t k = 0; k < kSsdvMaxErasures; ++k) era[k] = (uint8_t)key[k];
    for (uint32_t t = 0; t < kSsdvTrials; ++t) {
        uint32_t e = 0, ch = 0;
        if (!ssdv_trial(r, syn, era, 8u * t, w, &e, &ch)) continue;
        if (ssdv_crc_ok(w)) return accept(w, t, e, 8u * t, ch);
        *crc_bad += 1;
    }
    return false;
}

inline void ssdv_params_default(hd_ssdv_params* p) { p->max_fill = 7; p->_pad = 0; }
inline bool ssdv_params_ok(const hd_ssdv_params* p) { return p && p->max_fill <= 64u; }

// One stream's doors and delivery.  `words` holds the bytes from the absolute index `first` on, (c << 8) | b each: what a scan has not taken yet.
struct SsdvStream {
    uint32_t max_fill = 7;
    std::vector<uint32_t> words;
    uint64_t first = 0, n = 0, decided = 0, fillers = 0, crc_bad = 0, overlaps = 0, packets[5] = {0, 0, 0, 0, 0};
    bool has_prev = false, has_last = false;
    uint64_t prev_pos = 0, last_pos = 0;
    std::deque<hd_ssdv_packet> out;

    // (packets not yet taken stay)
    void reset()
    {
        words.clear();
        first = n = decided = fillers = crc_bad = overlaps = 0;
        for (uint64_t& p : packets) p = 0;
        has_prev = has_last = false;
        prev_pos = last_pos = 0;
    }
    void append(uint32_t b, uint32_t c) { words.push_back(std::min(c, kSsdvConfMax) << 8 | (b & 0xFFu)); n += 1; }
    void push_bytes(const uint8_t* b, const uint32_t* conf, size_t k)
    {
        for (size_t i = 0; i < k; ++i) append(b[i], conf ? conf[i] : kSsdvConfMax);
    }
    void push_records(const hd_clocked_record* r, size_t k, uint32_t char_len)
    {
        for (size_t i = 0; i < k; ++i) {
            if (char_len && has_prev && r[i].pos > prev_pos) {
                const uint64_t gap = (r[i].pos - prev_pos + char_len / 2u) / char_len;
                if (gap >= 2 && gap <= 1u + (uint64_t)max_fill) {
                    for (uint64_t q = 1; q < gap; ++q) append(0, 0);
                    fillers += gap - 1;
                }
            }
            has_prev = true; prev_pos = r[i].pos;
            uint32_t c = kSsdvConfMax;
            for (uint32_t q = 0; q < 8; ++q) {
                const int64_t v = r[i].data[q];
                c = std::min<uint32_t>(c, (uint32_t)std::min<int64_t>(v < 0 ? -v : v, kSsdvConfMax));
            }
            append(r[i].ch & 0xFFu, c);
        }
    }
    // A result of the scan, in increasing pos.
    void deliver(const hd_ssdv_packet& p)
    {
        if (has_last && p.pos < last_pos + 256u) { overlaps += 1; return; }
        has_last = true; last_pos = p.pos;
        packets[p.trial == HD_SSDV_NOFEC ? 4u : std::min<uint32_t>(p.trial, 3u)] += 1;
        out.push_back(p);
    }
    // out null: how many wait
    size_t take(hd_ssdv_packet* o, size_t cap)
    {
        if (!o) return out.size();
        size_t k = 0;
        for (; k < cap && !out.empty(); ++k) { o[k] = out.front(); out.pop_front(); }
        return k;
    }
    void stats(hd_ssdv_counters* c) const
    {
        c->bytes = n; c->decided = decided; c->fillers = fillers; c->crc_bad = crc_bad; c->overlaps = overlaps;
        for (int k = 0; k < 5; ++k) c->packets[k] = packets[k];
    }
    // the words in front of `upto` leave
    void drop(uint64_t upto)
    {
        if (upto <= first) return;
        words.erase(words.begin(), words.begin() + (size_t)std::min<uint64_t>(upto - first, words.size()));
        first = upto;
    }
    // The scan on the host: every position that is decided now.
    void scan()
    {
        while (decided + 256u <= n) {
            hd_ssdv_packet p;
            if (ssdv_decode(words.data() + (size_t)(decided - first), &p, &crc_bad)) { p.pos = decided; deliver(p); }
            decided += 1;
            if (decided - first >= 4096u) drop(decided);
        }
    }
};

}  // namespace hd
