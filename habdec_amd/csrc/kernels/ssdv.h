// SSDV packets (hd_ssdv_*, include/habdec_amd.h): the launchers of kernels/ssdv.hip and the layout both sides agree on.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/habdec_amd.h"

namespace hd {

constexpr uint32_t kSsdvRing = HD_SSDV_RING;                // a stream's newest bytes, one word (c << 8) | b each, slot = absolute index & (kSsdvRing - 1)
constexpr uint32_t kSsdvGuard = 16, kSsdvGuardWord = 0x55D7A11Cu;   // guard words in front of and behind every ring, the results and the counters
constexpr uint32_t kSsdvWaves = 4;                          // candidates (waves) per workgroup of k_ssdv_scan
constexpr uint32_t kSsdvAppendTile = 256;

// src[s], one round of a scan.  Append: stage_n new words at stage[stage_at ..] go to the ring slots from the absolute index append_pos on.  Scan: the
// round's candidates are the positions base .. base + n_total - 1, of which this launch takes the n from index off on.  Every word a candidate reads
// lies in the ring: the host appends at most kSsdvRing - 256 words to the at most 255 undecided ones.
struct SsdvSrc {
    uint64_t base, append_pos;
    uint32_t n_total, off, n;
    uint32_t stage_at, stage_n, _pad;
};
// One accepted candidate, 72 words: what comes back.  data: the 256 bytes of hd_ssdv_packet.data.
struct SsdvOut {
    uint64_t pos;
    uint32_t stream, trial, errors, erasures, changed, _pad;
    uint32_t data[64];
};
// The field's constants, made by the host (host/ssdv.hpp: SsdvField) when the object is created.  chien[k][l]: byte q is (1 / loc[l + 64 q])^k, the
// power a lane needs to evaluate a locator at its four positions; loc[j]: byte j's locator; rootmul[m][k]: root[m] * alpha^k, the eight multiples that
// make a product with root[m] out of ands and xors; root127[m] = root[m]^127.
struct SsdvTables {
    uint32_t chien[33][64];
    uint8_t loc[256];
    uint8_t rootmul[32][8];
    uint8_t root127[32];
};

// ring [S][ring_stride] uint32: kSsdvRing words behind kSsdvGuard guard words.  Grid (tiles of kSsdvAppendTile words over max_n, S).
void launch_ssdv_append(hipStream_t st, uint32_t n_streams, uint32_t max_n, const SsdvSrc* src, const uint32_t* stage, uint32_t* ring, size_t ring_stride);
// cnt: [0] the accepted candidates of the launch (the host clears it in front of one), [1 + s] stream s's crc_bad, both behind kSsdvGuard guard words
// (the pointer is to cnt[0]); out: out_cap results.  Grid (groups of kSsdvWaves candidates over cap, the longest n of the launch; S).
void launch_ssdv_scan(hipStream_t st, uint32_t n_streams, uint32_t cap, const SsdvSrc* src, const SsdvTables* tab, const uint32_t* ring, size_t ring_stride,
                      uint32_t* cnt, SsdvOut* out, uint32_t out_cap);

}  // namespace hd
