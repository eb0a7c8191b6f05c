// The engine's state, for the translation units of libhabdec_amd.so that work on an hd_engine: engine.cpp (the decode pipeline), wideband.cpp (survey,
// waterfall) and demod_rows.cpp (baud-rate probe, clocked decoder).  Internal: nothing here is part of the C ABI of include/habdec_amd.h.
#pragma once

#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/habdec_amd.h"
#include "dev_types.h"
#include "host/afc_tracker.hpp"
#include "host/decim_plan.hpp"
#include "host/fir_design.hpp"
#include "host/fir_lds.hpp"
#include "host/format_trial.hpp"
#include "host/text_stage.hpp"
#include "kernels/launch.h"
#include "kernels/spectrum_math.h"

struct hd_engine;

namespace hd { namespace eng {

// Defined in engine.cpp.  fail: the message becomes the calling thread's hd_last_error.
int fail(int code, const std::string& msg);
int check_stream(const hd_engine* e, uint32_t s);
int flush_locked(hd_engine* e);          // the calls in flight are delivered (the engine's mutex is held)

#define HD_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return hd::eng::fail(HD_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count)
    {
        hipError_t e = alloc_unfilled(count);
        if (e == hipSuccess) e = hipMemset(p, 0, std::max<size_t>(count, 1) * sizeof(T));
        return e;
    }
    // For what its owner fills itself, by a clear or a copy on its own queue: nothing is written here, and nothing runs on the null stream.
    hipError_t alloc_unfilled(size_t count)
    {
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
        n = e == hipSuccess ? count : 0;
        return e;
    }
    // At least `count` elements.  Where it grows, the old memory is freed first and the contents are not kept.
    hipError_t grow(size_t count)
    {
        if (count <= n) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; }
        return alloc_unfilled(count);
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// `rows` rows of guard | payload | guard in device memory, the one layout every kernel with guarded arrays assumes: G 32-bit words of `pattern` on either
// side of each row's payload, so a row is payload + 2 G 4 / sizeof(T) elements of T.  (A payload is a whole number of 32-bit words.)
template <typename T>
struct Guarded {
    static constexpr size_t stride_of(size_t payload, uint32_t G) { return payload + 2 * (size_t)G * sizeof(uint32_t) / sizeof(T); }
    DevBuf<T> buf;
    size_t stride = 0;                     // a row, guards included, in elements: what the kernels take beside base()
    uint32_t G = 0, pattern = 0;
    // The allocation, and one fill of the whole array with the pattern on `queue` (not waited for): the payloads are the owner's to clear.
    hipError_t alloc(size_t rows, size_t payload, uint32_t guard_words, uint32_t guard_pattern, hipStream_t queue)
    {
        G = guard_words; pattern = guard_pattern;
        stride = stride_of(payload, G);
        hipError_t e = buf.alloc_unfilled(rows * stride);
        if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(buf.p), (int)pattern, rows * stride * sizeof(T) / sizeof(uint32_t), queue);
        return e;
    }
    T* base() const { return buf.p; }
    T* row(size_t r) const { return buf.p + r * stride + G * sizeof(uint32_t) / sizeof(T); }     // row r's payload
    const uint32_t* guard_front(size_t r) const { return reinterpret_cast<const uint32_t*>(buf.p + r * stride); }
    const uint32_t* guard_back(size_t r) const { return reinterpret_cast<const uint32_t*>(buf.p + (r + 1) * stride) - G; }
};

// The guards of one row of a guarded array of any element, for the test hooks' counter (demod_rows.cpp: damaged_guards).
struct GuardedRow {
    const uint32_t *front, *back;
    uint32_t G, pattern;
    template <typename T>
    GuardedRow(const Guarded<T>& a, size_t r) : front(a.guard_front(r)), back(a.guard_back(r)), G(a.G), pattern(a.pattern) {}
};

template <typename T>
struct PinBuf {
    T* p = nullptr;
    T* dev = nullptr;      // the same memory as the GPU addresses it (kernels write results straight into it)
    size_t n = 0;
    hipError_t alloc(size_t count)
    {
        n = count;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) std::memset(p, 0, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), p, 0);
        return e;
    }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
};

// The size bookkeeping mirrored from the reference that one call advances.  plan_call computes every stream's next state into
// hd_engine::mirror_next; commit_call makes it the current one (hd_engine::mirror) once the call is enqueued -- a refused call leaves it as it was.
struct SizeState {
    size_t stage_buf[2] = {0, 0};   // Decimator::p_buff_.size()
    size_t pending = 0;             // iq_samples_decimated_.size()
    size_t fft_fill = 0;            // freq_in_.size()
    size_t fir_buf = 0;             // FirFilter::buff_.size()
    uint32_t fir_T_run = 0;         // tap count of the last low-pass run (FirHistory, dev_types.h)
    uint32_t head_n = 0;            // FirHistory head, lazily: how many samples of the last run's input a later run may ask for ...
    uint64_t head_call = ~0ull;     // ... the call that run was in (its input sits in THAT call's low-pass buffer until the buffer's turn comes again) ...
    bool head_aside = false;        // ... or: the head has been copied to the side buffer (the stream did not run in the call behind its last run)
    uint32_t tune_phase = 0;        // tuning phase of the next call to be submitted
    uint32_t front_phase = 0;       // ... and the phase of the tuning at the input rate (hd_stream_set_front_tune)
    uint32_t win_ub = 0, inflight_m = 0;   // upper bound of backlog samples without final window results; low-pass outputs of undelivered calls (collect() learns them back)
    uint32_t last_n2 = 0, last_pend_before = 0, last_m = 0;   // last call (for the getters)
    int last_buf = 0;
    uint8_t fft_buf = 0;            // which of the stream's two spectrum collection buffers the next call appends to (dev_types.h sc_fft_buf; always 0 unless hd_engine::lazy_spectra)
    uint8_t spec_buf = 0;           // ... and the one that completed last
    bool spec_stale = false;        // the spectrum of that buffer has not been stored into `spec` / `power`: the tail that transformed it kept the statistics only (refresh_spectra)
    bool demod_in_ring = false;     // the last call's discriminator output was not stored into `demod`: it is the newest last_m samples of the symbol ring (fill_tail)
};

struct StreamHost {
    // control plane
    double baud = 300;
    float lp_bw = 1500, lp_trans = 0.025f;
    bool dc = false;
    hd::LowpassDesigner lp;
    bool taps_dirty = false;
    uint32_t tune_step = 0;         // tuning step of the next call to be submitted (hd_stream_set_tune; its phase: SizeState::tune_phase)
    // data-dependent state learned back from the device
    uint32_t held = 0;
    bool sym_reset = true;          // symbol parameters changed since the window cache was built
    // host stages
    hd::TextStage text;
    hd::AfcTracker afc;
    hd::SpectrumStats stats{};
    bool have_spectrum = false;     // freq_out_.size() == 4096
    uint64_t spectra = 0;
    // last call delivered (for the getters)
    uint32_t last_nbits = 0, last_nflips = 0;
    uint64_t flip_list_full = 0;   // calls in which the device's flip list filled up (kMaxFlipsPerCall) and the search went on a call later
    uint64_t bits_total = 0;
    std::vector<uint32_t> last_words;
    uint32_t demod_ck[2] = {0, 0}, demod_ck_n = 0xFFFFFFFFu;   // discriminator checksum of the call delivered last (BitsHeader::demod_ck)
    uint64_t demod_ck_call = 0;                               // ... and that call's index (0 = the engine's first hd_process_* call)
    uint64_t demod_ck_hash = 0xCBF29CE484222325ull;           // every delivered call's (n, ck[0], ck[1]) folded into one word (hd_stream_demod_checksum_total)
    uint64_t demod_ck_calls = 0, demod_ck_unknown = 0;        // calls folded in / calls whose slot carried no checksum (0: every route fills it)
    // digital tuning of the decimated chunk (hd_stream_set_tune, kernels/tune.h) and the closed loop over it (hd_stream_set_auto_afc)
    double tune_hz = 0;
    uint64_t tune_from = 0, retunes = 0;      // first call of the current offset; automatic retunes so far
    bool auto_afc = false;
    double afc_hold_s = 6.0, afc_min_hz = 100.0;
    uint64_t afc_elapsed = 0;                 // input samples delivered since the loop was set or last retuned
    // tuning at the input rate, in front of the first decimation stage (hd_stream_set_front_tune; its phase: SizeState::front_phase)
    double front_hz = 0;
    uint32_t front_step = 0;
    uint64_t front_from = 0;                  // first call of the current offset
    // framing trial (hd_stream_set_format_trial): four text stages beside `text`, fed the same bits at delivery; null while off
    std::shared_ptr<hd::FormatTrial> trial;     // (shared: a StreamHost is copied where a setter tries a value out)
};

} }  // namespace hd::eng

using hd::eng::fail;
using hd::eng::check_stream;
using hd::eng::flush_locked;
using hd::eng::DevBuf;
using hd::eng::PinBuf;
using hd::eng::Guarded;
using hd::eng::GuardedRow;
using hd::eng::SizeState;
using hd::eng::StreamHost;

struct hd_engine {
    hd_engine_config cfg{};
    double fs = 0, fsd = 0;
    std::vector<hd::DecimStage> stages;
    uint32_t S = 0, D = 1;
    uint32_t n1_cap = 0, n2_cap = 0;        // per-call capacities after stage 1 / last stage
    uint32_t taps_cap = 0, fir_hist_cap = 0; // low-pass tap capacity, history slots in front of the pending samples
    size_t lds_per_wg = 0;                   // LDS the device grants one workgroup (queried at creation)
    uint32_t lp_taps_max = 0;                // longest low-pass a call may run: k_fir_demod's LDS image inside lds_per_wg (host/fir_lds.hpp), at most kTapsPrevMax
    size_t fbuf_stride = 0;
    uint32_t tail_cap = 0, backlog_cap = 0, slot_words = 0, flips_cap = 0, max_R = 0, min_R = 4;
    int bins_sep = 8;
    bool decode_enabled = true;
    bool fast = false;         // hd_engine_config.arith == HD_ARITH_FAST: the hd::fast kernels (fused multiply-add in every FIR; tolerance 1e-5, not bit-identical floats)
    bool one_stream = false;
    bool lazy_spectra = false; // batch mode: the stream tails store a spectrum's AFC statistics only; `spec` / `power` are filled when a getter asks (refresh_spectra).  HD_EAGER_SPECTRA=1: stored by every tail
    bool no_tail = false;      // HD_NO_TAIL: never use the one-wave stream tail (kernels/tail_body.h); A/B measurements
    uint32_t tail_max_n2 = 2048;   // HD_TAIL_MAX_N2: most decimated samples per call for which the stream tail is used
    int last_route = -1;       // route of the previous call (Route; the routes use the stage-2 buffers on different queues)
    // Step mode (batch decoding, kernels/decimate.hip k_step): the stream tails of call k ride in the stage-1 launch of call k+1.
    struct PendingTail { bool valid = false; hd::TailArgs ta{}; int slot = 0; int r2 = 0, t2 = 0; } pend;
    DevBuf<float2> fft_tw;     // [64][64] the transform's twiddles, lane-major (kernels/spectrum_math.h: fft_twiddles), rounded once from double
    bool no_claim = false;     // HD_NO_CLAIM: step launches with fixed shares of tiles (A/B measurements)
    uint32_t step_run = 0;     // HD_STEP_RUN: tiles per drawn run (default 4, minimum 2)
    bool no_cu_step = false;   // HD_NO_CU_STEP: step launches as single-wave workgroups (k_step) instead of one workgroup per CU (k_step_cu)
    uint32_t ring_run = 0;     // HD_RING_RUN: tiles per drawn run of the per-CU ring kernels (default: pick_ring_run)
    uint32_t ring_chain = 1;   // HD_RING_CHAIN: 0 = the /32 worker waves' tiles all stand alone (the plain schedule: 64 - HR outputs per tile); default: chained runs (host/ring_schedule.hpp)
    uint32_t ring_short_pct = 25;   // HD_RING_SHORT_PCT: share of an XCD's tiles the worker waves draw as SINGLE tiles at the end of a launch (guided hand-out; 0 = whole runs to the end)
    bool ring_short_set = false;    // ... was given.  Not given, chained launches take an eighth of the streams, not a quarter (make_claim)
#ifndef HD_S1_SLOTS_BATCH
#define HD_S1_SLOTS_BATCH 4
#endif
    static constexpr uint32_t kS1Slots = HD_S1_SLOTS_BATCH;     // tile slots of k_stage1_cu in batch mode on the separate-kernels path: four leave half of a CU's LDS to the back-half
                                                // workgroups of the previous call on the other queue (/16: 0.334-0.343 ms per step against 0.342-0.351 with eight)
    PinBuf<unsigned int> ring_gave_up;     // mapped host word a wave of k_step_cu / k_stage1_cu sets when a bounded wait runs out (never in a correct run)
    std::string fail_cause;                // what put the engine into its failed state (reported again by every later call)
    bool device_failed = false;            // ... after which the engine stays failed: the launch that gave up left stage-1 output incomplete, and up to
                                           // three calls are undelivered by the time a collect() sees the word -- which of them it was cannot be told
    uint64_t step_launches = 0;
    DevBuf<unsigned int> step_ctr;         // two sets of per-XCD run counters ([2][16][32] u32), alternating per step launch
    uint32_t pend_max_taps = 0;
    bool dec_wgs_forced = false;   // HD_DEC_WGS_PER_CU was given (tests of the linear split)
    // Timing experiments (results wrong: step launches without their tails -- 1 -- or without stage 1 -- 2; tools/micro/joules.py) exist in a VARIANT build only
    // (-DHD_TIMING_EXPERIMENT, HD_BUILD_VARIANT=timingexp: reads HD_CU_EXP): no environment variable makes the product library skip the result-slot tag
    // check or deliver wrong results.
#ifdef HD_TIMING_EXPERIMENT
    int cu_exp = 0;
#else
    static constexpr int cu_exp = 0;
#endif
    uint32_t n_cus = 0, dec_wgs_per_cu = 0;   // stage-1 linear split: workgroups per CU (0 = classic grid), see kernels/decimate.hip
    hipStream_t qa = nullptr, qb = nullptr, qc = nullptr;   // front (decimation, spectrum) and back (FIR, symbols, results) HIP streams
    // hd_process_host: copies run on their own stream into two alternating slabs; a call returns once ITS copy has landed, so the
    // caller may reuse (or free) the buffer at once, like Decoder::pushSamples' copy -- whatever the engine still has queued.
    hipStream_t qh = nullptr;
    DevBuf<float2> staging2;
    hipEvent_t ev_copy[2] = {nullptr, nullptr}, ev_staging_free[2] = {nullptr, nullptr};
    bool staging_used[2] = {false, false};
    uint64_t host_calls = 0, host_calls_in_place = 0;   // hd_process_host calls through the staging slabs / served in place from page-locked memory
    // hd_process_*_fmt: a packed call is unpacked into the staging slab of its turn (kernels/iq_unpack.hip) and goes on as a cf32 call on that slab -- on
    // qh, or on a synchronous engine's own queue where there is nothing to copy.  packed[j]: where the packed bytes of a pageable (or batch-mode) host
    // buffer land first, [S][max_chunk] samples of the widest format seen so far, allocated on first use; unpack_n: the call's per-stream counts for the
    // kernel (one array: the unpack that read it is done when its call returns).
    unsigned char* packed[2] = {nullptr, nullptr};
    size_t packed_bytes[2] = {0, 0};
    DevBuf<uint32_t> unpack_n;
    uint32_t timing_every = 8;   // HIP-event timing on every Nth call (0 = off): each event record is a barrier packet worth ~6 us of queue time
    hd_timing last_timing{};
    // Fast mode, long low-pass filters (>= kLpFftMinTaps taps: configs[4]'s 4097): the filter as transforms (kernels/fir_demod.hip: k_lp_gather / k_lp_mul around
    // rocFFT, k_fir_demod with the filtered samples handed in).  Two transform lengths, the smaller one where [history | inputs] of every stream fits it.
    static constexpr uint32_t kLpFftMinTaps = 1024;
    uint32_t lpf_N[2] = {0, 0};
    rocfft_plan lpf_fwd[2] = {nullptr, nullptr}, lpf_inv[2] = {nullptr, nullptr};
    rocfft_execution_info lpf_info = nullptr;
    DevBuf<char> lpf_workbuf;
    DevBuf<float2> lpf_x, lpf_k;           // [S][lpf_N[1]]: the input images / filtered samples of the call in the back half; the taps' spectra
    DevBuf<uint32_t> lpf_flags;            // [S][2]: the tag (CallSlot::seq, never 0) of the last call whose block held a sample exactly zero / any other sample (fir_demod.hip k_lp_gather)
    PinBuf<uint32_t> lpf_ntaps;            // [S]: tap counts the spectra in lpf_k were made from
    uint32_t lpf_k_N = 0;                  // ... and the transform length (0: none yet)
    bool lpf_k_stale = true;
    uint64_t lpf_calls = 0;

    DevBuf<float2> staging, dec1, dec1b, dec1c, hist1[2], hist2[2], fbuf[3], fft_in, spec, filtered;   // dec1/b/c: stage-1 output, rotating per call
    DevBuf<float> stage_taps[2], lp_taps, power, demod, tail, weight;
    DevBuf<unsigned long long> flipmask;
    DevBuf<uint32_t> flips_dbg;
    DevBuf<hd::SymState> d_symstate;
    DevBuf<hd::DemodCarry> carry[2];
    DevBuf<float2> fir_head;          // [S][head_cap]: FirHistory heads moved aside -- the first samples of a stream's last low-pass run's input, copied here by the first call in
                                      // which the stream did not run (dev_types.h: the head, lazily); a stream that ran in the previous call finds them in that call's buffer
    DevBuf<float> tune_tab;           // the phasor tables [C | F] of the per-stream tuning (kernels/tune.h), 2 x 256 (cos, sin)
    DevBuf<uint32_t> demod_ck_acc;    // [S][2]: the discriminator checksum of the call in the back half of the separate-kernels path (k_fir_demod adds, k_symbols collects and clears)
    uint32_t head_cap = 0;
    DevBuf<hd::SymbolParams> d_sym;
    PinBuf<hd::SymbolParams> h_sym;
    PinBuf<hd::StreamCall> h_spec_call;   // [S], lazy_spectra: the parameter block of the spectrum launch a getter triggers (only fft_run is set: which streams, which buffer)
    // Everything a call in flight owns, double-buffered so call k+1 can be enqueued (and its front half can run)
    // while call k's back half is still executing and its results have not been read yet.
    static constexpr int kSlots = 4;   // calls whose host-visible blocks (parameters, result slots, spectrum statistics) may be in use at once: in flight + being delivered
    struct CallSlot {
        DevBuf<hd::StreamCall> d_call;
        PinBuf<hd::StreamCall> h_call;
        PinBuf<uint32_t> h_slots;                 // written by the symbol scan kernel over PCIe (zero-copy), read after ev_done
        PinBuf<hd::SpectrumStatsDev> h_stats;    // written by the spectrum kernel
        PinBuf<uint2> h_tune;                     // (step, phase) of every stream for this call, read by the kernels in place; passed only when some stream is tuned
        PinBuf<uint2> h_front;                    // the same for the tuning at the input rate: read in place by k_decimate_tuned, which runs only when some stream has one
        bool timed = false, timed_step = false;   // this call carries the timing events (a step call: only the two around its one launch)
        hipEvent_t ev_front = nullptr, ev_done = nullptr, ev_params = nullptr, ev_spec = nullptr, t0 = nullptr, t1 = nullptr, t2 = nullptr, t3 = nullptr;
        bool busy = false;
        uint32_t seq = 0;                         // this call's tag: what every result slot's BitsHeader::seq must read before the slot is taken as delivered
        uint64_t total_in = 0;
        uint32_t r1 = 1;
        ~CallSlot() { for (hipEvent_t ev : {ev_front, ev_done, ev_params, ev_spec, t0, t1, t2, t3}) if (ev) (void)hipEventDestroy(ev); }
    } slot[kSlots];
    uint64_t calls = 0;
    uint64_t delivered = 0;   // calls whose results have been delivered; calls - delivered <= 2 (pipelined mode)
    int cur = 0;          // which fbuf receives this call's chunk (three take turns: the one a call writes was last read by the back half of call k-3, which the host has collected)
    int hist_cur = 0;     // which stage-history buffers are read this call (the others are written)
    int carry_cur = 0;
    bool sym_dirty = true;

    std::vector<StreamHost> st;
    std::vector<SizeState> mirror, mirror_next;   // [S]: the streams' size bookkeeping; the call being planned (swapped in by commit_call)
    std::recursive_mutex mtx;   // recursive: a sentence / character callback (fired under it, on the calling thread) may call the text getters
    bool in_callback = false;   // ... but not the data getters that would have to flush the pipeline from inside a delivery
    hd_sentence_cb sentence_cb = nullptr; void* sentence_user = nullptr;
    hd_match_cb match_cb = nullptr; void* match_user = nullptr;
    hd_chars_cb chars_cb = nullptr; void* chars_user = nullptr;
    uint64_t sentences_ok = 0;

    ~hd_engine()
    {
        for (rocfft_plan pl : {lpf_fwd[0], lpf_fwd[1], lpf_inv[0], lpf_inv[1]}) if (pl) rocfft_plan_destroy(pl);
        if (lpf_info) rocfft_execution_info_destroy(lpf_info);
        if (qa) (void)hipStreamDestroy(qa);
        if (qb && qb != qa) (void)hipStreamDestroy(qb);
        if (qc && qc != qa) (void)hipStreamDestroy(qc);
        if (qh) (void)hipStreamDestroy(qh);
        for (unsigned char* pk : packed) if (pk) (void)hipFree(pk);
        for (hipEvent_t ev : {ev_copy[0], ev_copy[1], ev_staging_free[0], ev_staging_free[1]}) if (ev) (void)hipEventDestroy(ev);
    }
};

namespace hd { namespace eng {

inline int failed_state(const hd_engine* e) { return fail(HD_ERR_DEVICE, "this engine is in its failed state (" + e->fail_cause + ") -- destroy the engine"); }

// Every call on one of the objects beside the pipeline (survey, waterfall, baud-rate probe, clocked decoder) starts here, under the engine's mutex.
inline int enter(const hd_engine* e)
{
    if (e->device_failed) return failed_state(e);
    HD_HIP(hipSetDevice(e->cfg.device));
    return HD_OK;
}

// What a kernel reads must be memory the GPU can address: a host pointer HIP does not know never reaches a launch.
inline bool is_device_pointer(const void* p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged &&
                                                          !(at.type == hipMemoryTypeHost && at.devicePointer))) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

// The transform's twiddles for an object beside the pipeline: the engine's, or, where the engine computes no spectra and holds none, the same table
// uploaded into `own` on q.  host: where that table is made, the creator's local -- the upload is enqueued, not waited for.
inline int engine_or_own_twiddles(const hd_engine* e, DevBuf<float2>& own, std::vector<float2>& host, hipStream_t q, const float2** tw)
{
    *tw = e->fft_tw.p;
    if (*tw) return HD_OK;
    host.resize(hd::kFftBins);
    hd::specwave::fft_twiddles(host.data());
    HD_HIP(own.alloc_unfilled(host.size()));
    HD_HIP(hipMemcpyAsync(own.p, host.data(), host.size() * sizeof(float2), hipMemcpyHostToDevice, q));
    *tw = own.p;
    return HD_OK;
}

} }  // namespace hd::eng
