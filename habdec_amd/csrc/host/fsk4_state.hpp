// The 4FSK modem's per-stream state and layouts (hd_fsk4_*, include/habdec_amd.h): one set of structs for kernels/fsk4.hip and its restatement host/fsk4.hpp.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define HD_FSK4_BOTH __host__ __device__
#else
#define HD_FSK4_BOTH
#endif

namespace hd {

struct Fsk4State {
    uint64_t n;                // samples pushed
    uint64_t g;                // slots written: every slot whose last sample is below n
    uint32_t F;                // 0: the stream has no modem
    uint32_t W;
    uint32_t phi[4];
    uint32_t psi[4];           // the tones' phase words: 0 after set_modem and reset, moved by every retune so that the rotators' phases are continuous
    uint32_t tot[8];           // sums of r_re, r_im of tone 0, then of tones 1 .. 3, over j < n, mod 2^32
};
static_assert(sizeof(Fsk4State) == 88, "fsk4 state layout: phi and psi lie together, a retune copies them in one piece");
// A stream's history, kept as running sums like the tones object's: word (k & (kFsk4Ring32 - 1)) of ring t is tot[t] after k samples, for the newest
// kFsk4Ring32 values of k <= n.  W <= kFsk4Ring32.
constexpr uint32_t kFsk4Ring32 = 2048;
constexpr uint32_t kFsk4Guard = 16, kFsk4GuardWord = 0xF5C4F5C4u;   // guard words in front of and behind every ring, the counters and the results
constexpr uint32_t kFsk4MaxSymbols = 260, kFsk4MaxCodewords = 22, kFsk4MaxPayload = 32;
constexpr uint32_t kFsk4Settle = 16;                                 // slots behind a group's first candidate in which its members contest the delivery
constexpr int32_t kFsk4PadConfidence = 1 << 24;                     // the zero-padded data positions of the last codeword: hard 0, this sure

// The slots whose last sample lies below n: slot g's last sample is end(g) = ((g + 8) F >> 19) - 1, strictly increasing in g since F >= 8 * 65536.
// end(g) < n  <=>  (g + 8) F < (n + 1) 2^19  <=>  g + 8 < ceil((n + 1) 2^19 / F).  (n < 2^44: a century at a decimated rate of 4 kS/s.)
HD_FSK4_BOTH inline uint64_t fsk4_slots_before(uint32_t F, uint64_t n)
{
    const uint64_t c = (((n + 1u) << 19) + F - 1u) / F;
    return c > 8u ? c - 8u : 0u;
}
HD_FSK4_BOTH inline uint64_t fsk4_slot_end(uint32_t F, uint64_t g) { return (((g + 8u) * (uint64_t)F) >> 19) - 1u; }

// The remainder of a 23-bit word by the generator (degree 11, 12 bits): its syndrome, 11 bits.
HD_FSK4_BOTH inline uint32_t fsk4_rem(uint32_t w, uint32_t poly)
{
    for (int b = 22; b >= 11; --b)
        if ((w >> b) & 1u) w ^= poly << (b - 11);
    return w & 0x7FFu;
}
// CRC16-CCITT, polynomial 0x1021, one byte into the register (initial value 0xFFFF, nothing reflected, no final xor)
HD_FSK4_BOTH inline uint32_t fsk4_crc16_byte(uint32_t crc, uint32_t byte)
{
    crc ^= byte << 8;
    for (int k = 0; k < 8; ++k) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
    return crc;
}

// What the frame kernel knows of a stream's frame, made by the host when the modem is set (host/fsk4.hpp: fsk4_tables).  syn[s]: the error pattern
// of weight <= 3 whose remainder by the generator is s (the code is perfect: there is exactly one).  src[23 k + b]: where bit b of codeword k (b = 0 its
// most significant data bit, b = 22 its last parity bit) is on the air: bits 0 .. 9 the frame's on-air bit (2 m + 0 / 1: symbol m's high / low bit), bit
// 15 set where the scrambler turns it over; kFsk4SrcPad: a zero-padded data position.
constexpr uint16_t kFsk4SrcPad = 0xFFFFu;
struct Fsk4Tab {
    uint32_t syn[2048];
    uint16_t src[23 * kFsk4MaxCodewords + 6];      // (512 entries)
    uint32_t nsym, K, P, poly;
    uint32_t uw;                                   // the unique word's 16 bits, first on air in bit 15
    uint32_t _pad[3];
};

// src[s] of a frame launch: the scan's candidates of stream s start at the slots base .. base + n_total - 1, of which this launch takes the n from index off on.
struct Fsk4Cand {
    uint64_t base;
    uint32_t n_total, off, n, _pad;
};
// One candidate that passed the unique-word gate, 16 words: what comes back.
struct Fsk4Out {
    uint64_t slot, metric;
    uint32_t stream, crc_ok, corrected, uw_errors;
    uint8_t payload[kFsk4MaxPayload];
};

}  // namespace hd
