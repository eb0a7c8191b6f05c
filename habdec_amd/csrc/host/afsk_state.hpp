// The AFSK / AX.25 modem's per-stream state, layouts and the walk (hd_afsk_*, include/habdec_amd.h): one set for kernels/afsk.hip and its restatement
// host/afsk.hpp.  The walk -- unstuffing, the delayed CRC, the address check -- is said once here and compiled for both sides; what differs between them
// (where the levels come from, who walks which flip pattern) is theirs.  tests/afsk_model.py says all of it again in numpy.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define HD_AFSK_BOTH __host__ __device__
#else
#define HD_AFSK_BOTH
#endif

namespace hd {

struct AfskState {
    uint64_t n;                // samples pushed
    uint64_t g;                // slots written: every slot whose last sample is below n
    uint32_t F;                // 0: the stream has no modem
    uint32_t W;
    uint32_t phi[2];           // mark, space
    uint32_t tot[4];           // sums of r_re, r_im of the mark filter, then of the space filter, over j < n, mod 2^32
};
static_assert(sizeof(AfskState) == 48, "afsk state layout");
// A stream's history as running sums, like the 4FSK modem's: word (k & (kAfskRing32 - 1)) of ring t is tot[t] after k samples.  W <= kAfskRing32.
constexpr uint32_t kAfskRing32 = 2048;
constexpr uint32_t kAfskGuard = 16, kAfskGuardWord = 0xAF5CAF5Cu;   // guard words in front of and behind every ring, list, count and result row
constexpr uint32_t kAfskMaxFrame = 332, kAfskMinFrame = 17;
constexpr uint32_t kAfskBack = 64;                                   // slots in front of a candidate the gate reads: the flag's eight bits need nine levels
constexpr uint32_t kAfskSettle = 8;                                  // slots behind a group's first candidate in which its members contest the delivery
constexpr uint32_t kAfskMaxFlips = 4, kAfskMaxPatterns = 64;
constexpr uint32_t kAfskResidue = 0xF0B8u;                           // the CRC register after a frame and its own FCS

// The slots whose last sample lies below n, and a slot's last sample: the 4FSK modem's grid (host/fsk4_state.hpp has the derivation).
HD_AFSK_BOTH inline uint64_t afsk_slots_before(uint32_t F, uint64_t n)
{
    const uint64_t c = (((n + 1u) << 19) + F - 1u) / F;
    return c > 8u ? c - 8u : 0u;
}
HD_AFSK_BOTH inline uint64_t afsk_slot_end(uint32_t F, uint64_t g) { return (((g + 8u) * (uint64_t)F) >> 19) - 1u; }

// L of the definition: the bits a walk may take.
HD_AFSK_BOTH constexpr uint32_t afsk_walk_bits(uint32_t max_frame_bytes) { return (8u * max_frame_bytes * 6u + 4u) / 5u + 8u; }

// CRC-16/X-25, one bit into the register (reflected 0x8408; the register starts at 0xFFFF, the FCS is its complement)
HD_AFSK_BOTH inline uint32_t afsk_crc_bit(uint32_t crc, uint32_t bit) { return ((crc ^ bit) & 1u) ? (crc >> 1) ^ 0x8408u : crc >> 1; }

// A callsign byte: bit 0 clear, and byte >> 1 in 'A'-'Z', '0'-'9' or ' '.
HD_AFSK_BOTH inline bool afsk_callsign_byte(uint32_t b)
{
    const uint32_t c = b >> 1;
    return !(b & 1u) && ((c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == ' ');
}

// How a walk ended, and what it read.
constexpr uint32_t kAfskOpen = 0, kAfskAbort = 1, kAfskClose = 2;
struct AfskWalk {
    uint32_t kind;             // kAfskOpen / kAfskAbort / kAfskClose
    uint32_t at;               // the bit (counted from the flag's last bit, which is 0) that ended it; the limit for an open walk
    uint32_t bits;             // kept bits in front of the closing flag; 0 unless closed
    uint32_t shaped, fcs_ok, addr_ok, fcs;
};

// The walk over the bits 1 .. limit behind a flag.  level(r): the level of bit r, 0 or 1, r = 0 the flag's last bit.  put(i, byte): byte i of the
// frame as it completes (the bytes of the closing flag never complete one that counts: see below).  Kept bits go through a delay of seven, so that
// the 0 and the six ones of the closing flag never reach the bytes or the CRC; the CRC register runs over everything else, the frame's own FCS
// included, and must end at kAfskResidue.  The address check runs on the bytes as they complete: the field ends at the first byte with bit 0 set,
// whose index must be 7 m - 1, 2 <= m <= 10, and lie in front of the FCS; the first six bytes of every address are callsign bytes.
template <typename Level, typename Put>
HD_AFSK_BOTH inline AfskWalk afsk_walk(Level level, uint32_t limit, uint32_t max_frame_bytes, Put put)
{
    AfskWalk w{kAfskOpen, limit, 0u, 0u, 0u, 0u, 0u};
    uint32_t prev = level(0u), ones = 0, kept = 0, delay = 0, crc = 0xFFFFu, cur = 0, last16 = 0;
    uint32_t addr_end = 0xFFFFFFFFu;
    bool addr_bad = false;
    for (uint32_t r = 1; r <= limit; ++r) {
        const uint32_t lv = level(r), bit = lv == prev ? 1u : 0u;
        prev = lv;
        if (bit) {
            if (++ones == 7u) { w.kind = kAfskAbort; w.at = r; return w; }
        } else {
            const uint32_t was = ones;
            ones = 0;
            if (was == 5u) continue;                                  // a stuffed bit
            if (was == 6u) {                                          // the closing flag's last bit
                w.kind = kAfskClose; w.at = r;
                const uint32_t fed = kept >= 7u ? kept - 7u : 0u, bytes = fed >> 3;
                w.bits = fed;
                w.shaped = !(fed & 7u) && bytes >= kAfskMinFrame && bytes <= max_frame_bytes;
                w.fcs_ok = crc == kAfskResidue;
                w.fcs = last16;
                w.addr_ok = !addr_bad && addr_end != 0xFFFFFFFFu && addr_end + 2u < bytes;
                return w;
            }
        }
        // a kept bit: the one kept seven bits ago leaves the delay
        if (kept >= 7u) {
            const uint32_t out = (delay >> 6) & 1u, fed = kept - 7u;
            crc = afsk_crc_bit(crc, out);
            last16 = (last16 >> 1) | (out << 15);
            cur |= out << (fed & 7u);
            if ((fed & 7u) == 7u) {
                const uint32_t i = fed >> 3;
                if (addr_end == 0xFFFFFFFFu && !addr_bad) {
                    if (cur & 1u) {
                        if (i % 7u == 6u && i >= 13u && i <= 69u) addr_end = i; else addr_bad = true;
                    } else if (i % 7u < 6u ? !afsk_callsign_byte(cur) : i >= 69u) addr_bad = true;
                }
                put(i, cur);
                cur = 0;
            }
        }
        delay = ((delay << 1) | bit) & 0x7Fu;
        ++kept;
    }
    return w;
}

// The gate's descriptor: the scan's slots of stream s are base .. base + n - 1.  The gate writes how many of them end a flag into count[s] and their
// offsets from base, in increasing order, into the stream's list.
struct AfskGate {
    uint64_t base;
    uint32_t n, _pad;
};
// src[s] of a frame launch: of the n_total flags in the stream's list this launch takes the n from index off on; their records go to out[out_off ..].
struct AfskCand {
    uint64_t base;
    uint32_t n_total, off, n, out_off;
};
// The flip patterns, made by the host at create: pattern j flips the list positions whose bits are set in mask[j]; pattern 0 is the untouched one.
struct AfskPatterns {
    uint64_t mask[kAfskMaxPatterns];
    uint32_t count, list, max_frame_bytes, L;      // list: repair_bits, 0 where repair is off (count is 1 then)
};

}  // namespace hd
