// The tone-filter demodulator's per-stream state (hd_tones_*, include/habdec_amd.h): one struct for kernels/tones.hip and its restatement host/tones.hpp.
#pragma once
#include <cstdint>

namespace hd {

struct TonesState {
    uint64_t n;                // samples pushed
    uint64_t qtot;             // sum of T(j), j < n, mod 2^64
    uint32_t F;                // 0: the stream has no modem
    uint32_t full, W, L;
    uint32_t phi[2];           // Phi_hi, Phi_lo
    uint32_t tot[4];           // sums of r_re, r_im of the upper tone, then of the lower, over j < n, mod 2^32
    uint32_t _pad[2];
};
// A stream's history, kept as running sums: word (k & (kTonesRing32 - 1)) of rotation ring t is tot[t] after k samples, for the newest kTonesRing32 values
// of k <= n; the normaliser's ring holds qtot the same way.  A launch reads every lagged value it needs (k >= n + 1 - W, k >= n + 1 - L) before it writes
// its own sums over the oldest ones, so W <= kTonesRing32 and L <= kTonesRing64 entries are enough.
constexpr uint32_t kTonesRing32 = 2048, kTonesRing64 = 16384;
// guard words in front of and behind every ring and every output row (kTonesGuard 32-bit words; the 64-bit ring's guards are kTonesGuard / 2 of its words)
constexpr uint32_t kTonesGuard = 16, kTonesGuardWord = 0x70E5C0DEu;

}  // namespace hd
