// The clocked decoder's per-stream state (hd_clocked_*, include/habdec_amd.h): one struct for kernels/clocked.hip and its restatement host/clocked.hpp.
#pragma once
#include <cstdint>

namespace hd {

struct ClockedState {
    uint64_t n, p;             // samples pushed, cursor
    uint64_t chars, rejects, dropped;
    uint64_t written, taken;   // records appended / records taken or overwritten: the ring holds [taken, written)
    uint32_t F;                // 0: the stream is off
    uint32_t nbits, nstops, invert;
    uint32_t total;            // sum of q_i, i < n, mod 2^32
    uint32_t _pad;
};
// guard words in front of and behind a stream's rings; 32-bit words of a record (hd_clocked_record)
constexpr uint32_t kClockedGuard = 16, kClockedRecWords = 14, kClockedGuardWord = 0xC10C4EDDu;

}  // namespace hd
