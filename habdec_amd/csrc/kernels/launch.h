// Host-callable launchers of the gfx950 kernels (defined in kernels/*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../dev_types.h"
#include "../../../include/habdec_amd.h"
#include "../host/clocked_state.hpp"
#include "../host/ring_schedule.hpp"
#include "../host/tones_state.hpp"

namespace hd {

struct DemodCarry {        // per-stream discriminator carry (previous filtered sample), ping-ponged per call
    float re, im;
    uint32_t primed;       // 0 until the stream's first FIR batch (FSK2_Demod.h:35 static initialiser)
    uint32_t _pad;
};

// How the single-wave stage-1 workgroups of a launch (step launches, and stage 1 alone over equally sized pushes) get their tiles when they
// draw them (ctr != nullptr): per-XCD counters, one per 128-byte line
// (32 u32 apart), zero when the launch starts; every XCD resets its counter in ctr_next, the set the NEXT step launch uses.
struct StepClaim {
    unsigned int* ctr = nullptr;             // this launch's counters, [n_xcd][32]
    unsigned int* ctr_next = nullptr;        // the other set
    uint32_t n_xcd = 0, runs_per_xcd = 0, run_len = 0;
    // Worker-wave kernels (stage1_ring.h: ring_worker) only -- guided hand-out: tickets [0, short_from) are runs of run_len tiles, the tickets behind them
    // are SINGLE tiles, so that the end of a launch is ragged by one tile's time instead of one run's (runs_per_xcd counts the tickets of both kinds;
    // tiles_per_xcd = short_from * run_len + (runs_per_xcd - short_from)).  short_from = 0xFFFFFFFF: every ticket is a whole run.
    uint32_t short_from = 0xFFFFFFFFu, tiles_per_xcd = 0;
    // Worker-wave kernels of the /32 stages only -- chained tiles (host/ring_schedule.hpp).  chain_rl >= 2: the launch's streams divide among the XCDs,
    // chain_sx to each; the first chain_sc streams of a share are tiled with the chained schedule (runs of chain_rl tiles, one ticket per run), the
    // other chain_sx - chain_sc with the plain one and drawn tile by tile behind them (the guided hand-out).  A ticket is hd::ring_ticket of it,
    // runs_per_xcd = hd::ring_tickets; run_len, short_from and tiles_per_xcd are not looked at.  chain_rl = 0: the plain grid described above.
    uint32_t chain_rl = 0, chain_sx = 0, chain_sc = 0;
    uint32_t chain_nfull = 0, chain_kclose = 0, chain_ntp = 0;   // hd::RingSchedule::n_full and ::k_close of the chained schedule (chain_rl is its ::rl), ::ntiles of the plain one
};

// ---- the fused stream tail (tail_body.h / tail.hip): stage 2 + low-pass + discriminator + symbol extractor, one wave per stream
struct TailArgs {
    // stage 2 + low-pass + discriminator (same buffers and conventions as launch_decimate + launch_fir_demod)
    const float2* dec1; size_t dec1_stride;
    const float2* hist2_in; float2* hist2_out; const float* taps2;
    float2* fbuf; float2* fbuf_next; size_t fbuf_stride; uint32_t fir_hist_cap;
    const float* lp_taps; uint32_t taps_stride;
    float* demod /* or null: the call's discriminator output is not stored a second time -- it is ring[(base + held - fir_m + i) & (ring_cap - 1)] of the
                    stream's SymState once the tail has run, which is where hd_stream_demodulated then reads it (batch mode) */; size_t demod_stride; float2* filtered;
    const DemodCarry* carry_in; DemodCarry* carry_out;
    const StreamCall* call; float2* fft_in;
    float2* head_buf /* [S][head_cap]: FirHistory heads moved aside */; const float2* fbuf_prev /* the previous call's low-pass buffers (dev_types.h: FirHistory head, lazily) */; uint32_t head_cap, n_streams;
    // symbol extractor (same rings and state as launch_symbols)
    float* ring; uint32_t ring_cap; SymState* sym; unsigned long long* flipmask; float* wsum; const SymbolParams* sp;
    uint32_t* slots; uint32_t slot_words; uint32_t* flips_dbg; uint32_t flips_cap;
    uint32_t seq;                                   // the call's tag, stored last into the result slot (BitsHeader::seq)
    // spectrum of a stream whose 4096-sample buffer completes in this call, done by the tail itself when fft_tw != nullptr (spectrum_wave.h)
    const float2* fft_tw; float2* spec; float* power; SpectrumStatsDev* stats; double rate; int bins_sep;
    // LDS carve in bytes from the base of the workgroup's scratch (tail_layout)
    // (search phase, overlaying the stream windows: [header][flip list + run info][run-sum strips] at fixed offsets, then from dyn_off to lds_bytes a region
    // every stream carves for itself: the flag-mask image of its searchable backlog, a sample cache for the run sums, a window-sum cache for the edge search)
    uint32_t pend_max, f_off, v_off, ws_off, words_off, tp_off, h2_off, flips_off, fl_cap, strips_off, dyn_off, lds_bytes;
    uint32_t op;          // stage-2 outputs per lane and piece the carve was made for (tail_layout; launch_tail picks the kernel by it)
    // per-stream tuning (tune.h): (step, phase) of each stream for THIS call, or null when no stream of the call is tuned; the phasor tables [C | F]
    const uint2* tune; const float* tune_tab;
};

constexpr uint32_t kStepLdsBytes = 20480;   // LDS of a stage-1 workgroup slot (eight per CU): what a tail riding in the stage-1 launch may use

// ---- the launcher that does not depend on the arithmetic mode (spectrum_wave.hip)
// The spectrum step in one launch, one wave per stream; tw64: the lane-major twiddle table (spectrum_math.h: fft_twiddles).
void launch_spectrum_wave(hipStream_t st, uint32_t n_streams, const float2* fft_in, const float2* tw64, float2* spec, float* power,
                          SpectrumStatsDev* stats, const StreamCall* call, double rate, int bins_sep,
                          uint32_t seq /* the call's tag, stored last into every SpectrumStatsDev written (SpectrumStatsDev::seq) */,
                          const float2* chunk = nullptr /* the low-pass input buffers [S][chunk_stride]: streams with StreamCall::fft_run == 2 take their 4096 samples from the head of this call's decimated chunk */,
                          size_t chunk_stride = 0, uint32_t fir_hist_cap = 0);

// Packed IQ -> cf32 (iq_unpack.hip), grid (tiles, rows): row r reads n_per_row[r] (a DEVICE array; null: n_uniform) samples of `fmt` (HD_IQ_CS16 / CS8 / CU8)
// at src + r * src_stride * bytes-per-sample and writes them to dst + r * dst_stride; max_n = the largest count of the launch.  A shared row is
// n_rows = 1 with both strides unused.  A cs16 row may start on any 4-byte boundary, a cs8 / cu8 row on any 2-byte boundary.  false: unknown fmt.
bool launch_iq_unpack(hipStream_t st, int fmt, uint32_t n_rows, uint32_t max_n, const void* src, size_t src_stride, const uint32_t* n_per_row,
                      uint32_t n_uniform, float2* dst, size_t dst_stride);

// Baud-rate probe (baud_probe.hip), one workgroup of 1024 threads per stream.  src[s]: where stream s's discriminator output of this push lies -- n floats
// at p, or (ring_mask != 0) the n floats in front of the append position base + held of *sym in the symbol ring at p, indices taken & ring_mask; n = 0:
// the stream is not touched.  hdr [S], acc64 [S][2][1024] (P, Q), acc32 [S][5][1024] (NB, re, im, n, cur_block); F, scale, ctab: the 1024-entry tables of
// host/baud_probe.hpp (BaudProbeTables).
struct ProbeSrc {
    const float* p;
    const SymState* sym;
    uint32_t n, ring_mask;
};
void launch_baud_probe(hipStream_t st, uint32_t n_streams, const ProbeSrc* src, hd_baud_probe_stream_state* hdr, unsigned long long* acc64, uint32_t* acc32,
                       const uint32_t* F, const uint32_t* scale, const int32_t* ctab);

// Clocked decoder (clocked.hip), one wave per stream.  src[s]: the probe's descriptor with a window -- of the n_total floats of the push this launch
// takes the n from index off on (n <= HD_CLOCKED_CHUNK; n = 0: nothing is appended, and nothing can be decided that was not decided before).
// st [S]; ring [S][ring_stride] uint32, a stream's HD_CLOCKED_RING running sums behind kClockedGuard guard words; rec [S][rec_stride] uint32, its
// record_cap records of 14 words (hd_clocked_record) behind kClockedGuard guard words.
struct ClockedSrc {
    const float* p;
    const SymState* sym;
    uint32_t n_total, ring_mask, off, n;
};
// lds_words: words of LDS per wave, at least look + h + n of every stream that is on (host/clocked.hpp: clocked_window_words); false: more than the CU has.
bool launch_clocked(hipStream_t st, uint32_t n_streams, const ClockedSrc* src, ClockedState* state, uint32_t* ring, size_t ring_stride, uint32_t* rec,
                    size_t rec_stride, uint32_t record_cap, uint32_t lds_words);

// Tone-filter demodulator (tones.hip), one workgroup per stream.  src[s]: of the n_total cf32 samples of the push at p this launch takes the n from index
// off on (n <= cap <= HD_TONES_CHUNK; n = 0, or a stream without a modem: not touched) and writes as many floats from index off on into the stream's row.
// st [S]; ring32 [S][4][ring32_stride] uint32, a stream's four rings of kTonesRing32 running sums, each behind kTonesGuard guard words; ring64
// [S][ring64_stride] uint64, its kTonesRing64 running sums of the normaliser behind kTonesGuard / 2 guard words; ctab: the probe's cosine table; rows
// [S][row_stride] float, row_cap floats behind kTonesGuard guard words.  cap: the longest n of the launch, which sizes the LDS; false: more than the CU has.
struct TonesSrc {
    const float2* p;
    uint32_t n_total, off, n, _pad;
};
bool launch_tones(hipStream_t st, uint32_t n_streams, uint32_t cap, const TonesSrc* src, TonesState* state, uint32_t* ring32, size_t ring32_stride,
                  unsigned long long* ring64, size_t ring64_stride, const int32_t* ctab, float* rows, size_t row_stride, uint32_t row_cap);

// ---- launchers of the mode-dependent kernels, once per arithmetic mode (arith.h)
namespace exact {
#include "launch_decls.inc"
}
namespace fast {
#include "launch_decls.inc"
}

}  // namespace hd
