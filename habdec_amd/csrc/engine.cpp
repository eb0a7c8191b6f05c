// libhabdec_amd.so -- host side of the MI355X RTTY demodulation engine: the C ABI of include/habdec_amd.h.
//
// Responsibilities: mirror the reference Decoder's integer bookkeeping per stream (how many samples each stage
// sees, when histories restart, when the spectrum buffer completes, when the low-pass is redesigned:
// reference code/Decoder/Decoder.h:416-542), upload it as one small parameter array per call, launch the gfx950
// kernels over all streams on one HIP stream, fetch the packed bits and spectrum statistics, and run the host
// text stage (RTTY framing, sentence extraction, CRC, callbacks: Decoder.h:559-637) and the AFC state machine.
// There is no CPU fallback: without a gfx950 device and the kernels in this library hd_engine_create fails.
//
// The engine's state (struct hd_engine and what it is made of) is in engine_state.h, shared with the objects that work beside the pipeline:
// wideband.cpp (survey, waterfall) and demod_rows.cpp (baud-rate probe, clocked decoder).
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <condition_variable>
#include <thread>

#include "engine_state.h"
#include "host/iq_convert.hpp"
#include "host/iq_file_batch.hpp"
#include "host/tune_host.hpp"
#include "kernels/spectrum_math.h"

// A launcher (or layout helper) of the kernels that exist once per arithmetic mode (kernels/arith.h): hd::exact::fn or hd::fast::fn by the engine's mode.
#define HDK(fn, ...) (e->fast ? hd::fast::fn(__VA_ARGS__) : hd::exact::fn(__VA_ARGS__))

namespace {

thread_local std::string g_err;     // hd_last_error: one per thread, whichever translation unit refused the call

}  // namespace

int hd::eng::fail(int code, const std::string& msg) { g_err = msg; return code; }

int hd::eng::check_stream(const hd_engine* e, uint32_t s)
{
    if (!e) return fail(HD_ERR_INVALID, "null engine");
    if (s >= e->S) return fail(HD_ERR_INVALID, "stream index out of range");
    return HD_OK;
}

namespace {

std::once_flag g_rocfft_once;

hd::SymbolParams symbol_params(const hd_engine* e, const StreamHost& s)
{
    hd::SymbolParams p{};
    p.float_abs = e->cfg.lookup_mode ? 1u : 0u;
    p.min_held = 0xFFFFFFFFu;
    p.spb = 0; p.R = 4;
    if (e->fsd > 0 && s.baud > 0) {
        const double spb = std::round(e->fsd / s.baud);
        if (spb >= 1 && spb < 1e9) {
            p.spb = (uint32_t)spb;
            p.R = (uint32_t)std::max(4, int(p.spb / 4));
            p.min_held = (uint32_t)std::ceil(e->fsd / s.baud * 3);
        }
    }
    return p;
}

float cutoff_rel(const hd_engine* e, const StreamHost& s) { return (float)(s.lp_bw / e->fsd); }

}  // namespace

extern "C" {

const char* hd_last_error(void) { return g_err.c_str(); }

/* Smallest non-empty per-stream sample count hd_process_* accepts for a decimation factor: a multiple of the factor that covers the
 * history of every stage (shorter inputs are undefined behaviour in the reference, Q4).  0 = unsupported factor. */
uint32_t hd_min_chunk(uint32_t decimation)
{
    std::vector<hd::DecimStage> st;
    if (!hd::decim_plan(decimation, st)) return 0;
    uint64_t need = decimation ? decimation : 1;
    uint64_t r = 1;
    for (const auto& g : st) { need = std::max<uint64_t>(need, (uint64_t)(g.taps.size() - 1) * r); r *= (uint64_t)g.ratio; }
    const uint64_t d = decimation ? decimation : 1;
    return (uint32_t)((need + d - 1) / d * d);
}

void hd_engine_config_default(hd_engine_config* c)
{
    std::memset(c, 0, sizeof(*c));
    c->device = 0; c->n_streams = 1; c->max_chunk = 65536; c->sampling_rate = 2.048e6; c->decimation = 64;
    c->baud = 300; c->rtty_bits = 8; c->rtty_stops = 2; c->lowpass_bw_hz = 1500; c->lowpass_trans = 0.025f;
    c->dc_remove = 0; c->lookup_mode = 1; c->enable_spectrum = 1; c->ungated = 0; c->keep_filtered = 0; c->pipeline = 0; c->arith = HD_ARITH_EXACT;
}

int hd_engine_create(const hd_engine_config* cfg, hd_engine** out)
{
    if (!cfg || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->n_streams < 1) return fail(HD_ERR_INVALID, "n_streams must be >= 1");
    if (!(cfg->sampling_rate > 0)) return fail(HD_ERR_INVALID, "sampling_rate must be > 0");
    if (cfg->max_chunk < 1) return fail(HD_ERR_INVALID, "max_chunk must be >= 1");
    if (cfg->arith != HD_ARITH_EXACT && cfg->arith != HD_ARITH_FAST) return fail(HD_ERR_INVALID, "arith must be HD_ARITH_EXACT (0) or HD_ARITH_FAST (1)");
    std::unique_ptr<hd_engine> e(new hd_engine);
    e->cfg = *cfg;
    e->fast = cfg->arith == HD_ARITH_FAST;
    if (!hd::decim_plan(cfg->decimation, e->stages))
        return fail(HD_ERR_INVALID, "Unsupported decimation factor: " + std::to_string(cfg->decimation));   // Decoder.h:317-319
    e->S = cfg->n_streams;
    e->D = cfg->decimation;
    if (cfg->max_chunk % e->D) return fail(HD_ERR_INVALID, "max_chunk must be a multiple of the decimation factor");
    e->fs = (double)(float)cfg->sampling_rate;        // Decoder::init(const float) (Decoder.h:223-225)
    e->fsd = e->fs / (double)e->D;
    e->decode_enabled = cfg->ungated || !(e->fsd > 4 * 40e3);   // Decoder.h:522
    if (cfg->baud > 0 && e->fsd / cfg->baud < 3.5)
        return fail(HD_ERR_UNSUPPORTED, "symbol rate above a third of the decimated rate (fewer than 4 samples per bit): the symbol extractor's windows would overlap");
    {   // AFC::FindPeaks separation in bins (AFC.h:110-111, 299-300)
        const float rel = (float)(500.0f / e->fsd);
        e->bins_sep = std::max(8, (int)std::round((double)rel * (double)hd::kFftBins));
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device || cfg->device < 0)
        return fail(HD_ERR_DEVICE, "no HIP device " + std::to_string(cfg->device) + " (this library has no CPU path)");
    HD_HIP(hipSetDevice(cfg->device));
    HD_HIP(hipStreamCreateWithFlags(&e->qa, hipStreamNonBlocking));
    // Synchronous delivery (pipeline = 0) has nothing to overlap between calls: one queue, no cross-queue event between the front and the back half
    // (0.283 -> 0.268 ms per step at 1024 streams, 12 us of it the hop from one queue to the other).
    e->one_stream = cfg->pipeline == 0;
    e->no_tail = getenv("HD_NO_TAIL") != nullptr;
    { const char* v = getenv("HD_EAGER_SPECTRA"); e->lazy_spectra = cfg->pipeline >= 1 && cfg->enable_spectrum && !(v && atoi(v)); }
    e->no_claim = getenv("HD_NO_CLAIM") != nullptr;
    if (const char* v = getenv("HD_STEP_RUN")) e->step_run = (uint32_t)atoi(v);
    e->no_cu_step = getenv("HD_NO_CU_STEP") != nullptr;
    if (const char* v = getenv("HD_RING_RUN")) e->ring_run = (uint32_t)atoi(v);
    if (const char* v = getenv("HD_RING_CHAIN")) e->ring_chain = atoi(v) ? 1u : 0u;
    if (const char* v = getenv("HD_RING_SHORT_PCT")) { e->ring_short_pct = std::min<uint32_t>((uint32_t)atoi(v), 100u); e->ring_short_set = true; }
    if (const char* v = getenv("HD_TAIL_MAX_N2")) e->tail_max_n2 = (uint32_t)strtoul(v, nullptr, 0);
    {
        hipDeviceProp_t prop;
        HD_HIP(hipGetDeviceProperties(&prop, cfg->device));
        e->n_cus = (uint32_t)prop.multiProcessorCount;
        // The longest low-pass the engine runs: k_fir_demod keeps a tile's inputs for ALL taps in LDS, and a workgroup gets what the device grants one (with
        // the opt-in launch_fir_demod asks for above 64 KB) -- 18899 taps inside a gfx950 CU's 160 KB.  The exact mode takes that kernel for every run, the
        // fast mode for every run that starts a filter from zeros, so the one limit holds for both; plan_call refuses a longer design.
        int lds_block = 0, lds_optin = 0;
        HD_HIP(hipDeviceGetAttribute(&lds_block, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device));
        if (hipDeviceGetAttribute(&lds_optin, hipDeviceAttributeSharedMemPerBlockOptin, cfg->device) != hipSuccess) { (void)hipGetLastError(); lds_optin = 0; }
        e->lds_per_wg = (size_t)std::max(std::max(lds_block, lds_optin), 0);
        e->lp_taps_max = std::min<uint32_t>(hd::fir_demod_max_taps(e->lds_per_wg), hd::kTapsPrevMax);
        if (e->lp_taps_max < 161u) return fail(HD_ERR_DEVICE, "the device grants a workgroup " + std::to_string(e->lds_per_wg) + " bytes of LDS: too little for the low-pass kernel");
        // Stage 1 of equally sized pushes runs as a linear split over k workgroups per CU.  Synchronous mode: all eight LDS slots of a
        // CU (measured against the classic per-stream grid on the same box: 125 vs 137 us per launch; 12, 16, 24, 32, 64 per CU: 150,
        // 135, 141, 135, 132 us).  Batch mode when the step kernel does not apply: six, so that the previous call's back half, on the
        // second queue, finds room underneath.
        e->dec_wgs_per_cu = cfg->pipeline ? 6u : 8u;
        if (const char* v = getenv("HD_DEC_WGS_PER_CU")) { e->dec_wgs_per_cu = (uint32_t)atoi(v); e->dec_wgs_forced = true; }
#ifdef HD_TIMING_EXPERIMENT
        if (const char* v = getenv("HD_CU_EXP")) e->cu_exp = atoi(v);
#endif
    }
    for (hipEvent_t* ev : {&e->ev_copy[0], &e->ev_copy[1], &e->ev_staging_free[0], &e->ev_staging_free[1]}) HD_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    if (e->one_stream) e->qb = e->qc = e->qa;
    else {
        if (!e->qb) HD_HIP(hipStreamCreateWithFlags(&e->qb, hipStreamNonBlocking));
        HD_HIP(hipStreamCreateWithFlags(&e->qc, hipStreamNonBlocking));   // parameter fetches: tiny kernels that need not queue behind stage 1
    }
    for (auto& sl : e->slot) {
        // No system-scope fence at these events (hipEventDisableSystemFence): what queues hand each other on this device needs agent scope only, and with the
        // default flags every record wrote back and invalidated the L2s -- ~5 us of queue time per event between two step launches (kernel trace, round 4),
        // and a system-scope release on the dispatch that carries ev_done costs 2.8 % of a step (round 5, one box, alternating: 0.1316-0.1323 against
        // 0.1283-0.1285 ms).  What the HOST reads behind ev_done -- result slots, spectrum statistics, the give-up word -- lives in coherent mapped host memory and
        // is written straight over PCIe; HIP does not promise that an event without the fence orders those stores before the host's reads, so
        // collect() does not rely on it: every result slot carries the call's tag, stored last behind a wait for the writing wave's other stores
        // (BitsHeader::seq), and a slot counts as delivered when the host reads that tag.
        static const unsigned ev_flags = (unsigned)hipEventDisableSystemFence;
        HD_HIP(hipEventCreateWithFlags(&sl.ev_front, hipEventDisableTiming | ev_flags));
        HD_HIP(hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming | ev_flags));
        HD_HIP(hipEventCreateWithFlags(&sl.ev_params, hipEventDisableTiming | ev_flags));
        HD_HIP(hipEventCreateWithFlags(&sl.ev_spec, hipEventDisableTiming | ev_flags));
        for (hipEvent_t* ev : {&sl.t0, &sl.t1, &sl.t2, &sl.t3}) HD_HIP(hipEventCreateWithFlags(ev, ev_flags));
    }

    const uint32_t S = e->S;
    const uint32_t r0 = e->stages.size() > 0 ? e->stages[0].ratio : 1;
    e->n1_cap = cfg->max_chunk / r0;
    e->n2_cap = cfg->max_chunk / e->D;
    // low-pass tap capacity: the design clamps to the batch length m <= pending_max and forces odd (FirFilter.h:185-188)
    const uint32_t m_cap = ((e->n2_cap + hd::kFirBatch - 1) / hd::kFirBatch) * hd::kFirBatch + hd::kFirBatch;
    e->taps_cap = (m_cap | 1u) + 1u;
    e->fir_hist_cap = (e->taps_cap + 1u) & ~1u;       // even, so the chunk behind it stays 16-byte aligned
    e->fbuf_stride = (size_t)e->fir_hist_cap + hd::kFirBatch + e->n2_cap + 2;
    e->fbuf_stride = (e->fbuf_stride + 1) & ~(size_t)1;
    e->backlog_cap = hd::kVentLimit + 1 + m_cap;       // most samples the symbol extractor can hold (SymbolExtractor.h:116)
    e->tail_cap = 1u;                                  // per-stream symbol ring: power of two >= vent limit + one batch + slack
    while (e->tail_cap < hd::kVentLimit + 1 + m_cap + 1024) e->tail_cap <<= 1;

    e->st.resize(S);
    e->mirror.resize(S);
    e->mirror_next.resize(S);
    for (auto& s : e->st) {
        s.baud = cfg->baud; s.lp_bw = cfg->lowpass_bw_hz; s.lp_trans = cfg->lowpass_trans; s.dc = cfg->dc_remove != 0;
        s.text.framer.nbits = cfg->rtty_bits; s.text.framer.nstops = cfg->rtty_stops;
        s.lp.float_trig = cfg->lookup_mode != 0;
    }
    {   // result slot: header + packed bits.  bits per call <= 3*backlog/spb (SymbolExtractor run lengths)
        const hd::SymbolParams p = symbol_params(e.get(), e->st[0]);
        const uint32_t spb = std::max<uint32_t>(p.spb, 1);
        uint32_t bits = 3u * e->backlog_cap / spb + 64u;
        bits = std::max<uint32_t>(256u, (bits + 31u) & ~31u);
        e->slot_words = (uint32_t)(sizeof(hd::BitsHeader) / 4) + bits / 32;
        e->max_R = std::max<uint32_t>(p.R, 4);
        e->min_R = e->max_R;
    }
    e->flips_cap = cfg->keep_filtered ? 256 : 0;

    // device memory
    HD_HIP(e->staging.alloc((size_t)S * cfg->max_chunk));
    if (e->stages.size() == 2) for (auto* b : {&e->dec1, &e->dec1b, &e->dec1c}) HD_HIP(b->alloc((size_t)S * e->n1_cap));
    HD_HIP(e->step_ctr.alloc(2 * 16 * 32 + 32));
    HD_HIP(e->ring_gave_up.alloc(4));
    e->ring_gave_up.p[0] = 0;
    if (!e->no_claim && e->n_cus % 32u == 0) {
        // The drawn runs of the step launches are split by the hardware's XCC id (kernels/decimate.hip, stage1_ring.h): every id in
        // [0, n_cus / 32) must show up in a chip-filling grid and no other may.  A CU mask or a partition mode that breaks that
        // turns the draws off (fixed shares: slower, never wrong).
        const uint32_t n_xcd = e->n_cus / 32u;
        // (the allocations above clear their memory on the null stream, which a non-blocking stream does not wait for: without this
        // the clearing of step_ctr could land on top of the probe's answer -- seen in one test run of three as a silent fall-back to
        // fixed shares)
        HD_HIP(hipDeviceSynchronize());
        const uint32_t seen = HDK(probe_xcc_mask, e->qa, e->n_cus, e->step_ctr.p + 2 * 16 * 32);
        if (n_xcd > 16 || seen != (n_xcd >= 32 ? 0xFFFFFFFFu : (1u << n_xcd) - 1u)) e->no_claim = true;
    } else
        e->no_claim = true;
    if (e->stages.size() >= 1) {
        for (auto& h : e->hist1) HD_HIP(h.alloc((size_t)S * (e->stages[0].taps.size() - 1)));
        HD_HIP(e->stage_taps[0].alloc(e->stages[0].taps.size() + 1));       // (+1: the ring kernels read the taps as aligned pairs; the word behind an odd count is never used)
        HD_HIP(hipMemcpy(e->stage_taps[0].p, e->stages[0].taps.data(), e->stages[0].taps.size() * 4, hipMemcpyHostToDevice));
    }
    if (e->stages.size() == 2) {
        for (auto& h : e->hist2) HD_HIP(h.alloc((size_t)S * (e->stages[1].taps.size() - 1)));
        HD_HIP(e->stage_taps[1].alloc(e->stages[1].taps.size() + 1));
        HD_HIP(hipMemcpy(e->stage_taps[1].p, e->stages[1].taps.data(), e->stages[1].taps.size() * 4, hipMemcpyHostToDevice));
    }
    for (auto& b : e->fbuf) HD_HIP(b.alloc((size_t)S * e->fbuf_stride));
    HD_HIP(e->lp_taps.alloc((size_t)S * e->taps_cap));
    HD_HIP(e->demod.alloc((size_t)S * m_cap));
    if (cfg->keep_filtered) HD_HIP(e->filtered.alloc((size_t)S * m_cap));
    HD_HIP(e->tail.alloc((size_t)S * e->tail_cap));
    HD_HIP(e->weight.alloc((size_t)S * e->tail_cap));
    HD_HIP(e->flipmask.alloc((size_t)S * (e->tail_cap / 64)));
    HD_HIP(e->d_symstate.alloc(S));
    if (e->flips_cap) HD_HIP(e->flips_dbg.alloc((size_t)S * e->flips_cap));
    for (auto& c : e->carry) HD_HIP(c.alloc(S));
    e->head_cap = std::min<uint32_t>(e->taps_cap, 8192u);   // a tap-count jump of more than 8192 reads zeros beyond (documented)
    HD_HIP(e->fir_head.alloc((size_t)S * e->head_cap));
    HD_HIP(e->demod_ck_acc.alloc((size_t)2 * S));
    HD_HIP(e->d_sym.alloc(S));
    HD_HIP(e->h_sym.alloc(S));
    for (auto& sl : e->slot) {
        HD_HIP(sl.d_call.alloc(S));
        HD_HIP(sl.h_call.alloc(S));
        HD_HIP(sl.h_slots.alloc((size_t)S * e->slot_words));
        HD_HIP(sl.h_tune.alloc(S));
        HD_HIP(sl.h_front.alloc(S));
    }
    {
        std::vector<float> tab(4 * hd::kTuneTable);
        hd::tune_tables(tab.data(), tab.data() + 2 * hd::kTuneTable);
        HD_HIP(e->tune_tab.alloc(tab.size()));
        HD_HIP(hipMemcpy(e->tune_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (cfg->enable_spectrum) {
        HD_HIP(e->fft_in.alloc((size_t)S * 2 * hd::kFftBins));        // two collection buffers per stream (dev_types.h sc_fft_row)
        if (e->lazy_spectra) HD_HIP(e->h_spec_call.alloc(S));
        HD_HIP(e->spec.alloc((size_t)S * hd::kFftBins));
        HD_HIP(e->power.alloc((size_t)S * hd::kFftBins));
        for (auto& sl : e->slot) HD_HIP(sl.h_stats.alloc(S));
        {
            std::vector<float2> tw(hd::kFftBins);
            hd::specwave::fft_twiddles(tw.data());
            HD_HIP(e->fft_tw.alloc(hd::kFftBins));
            HD_HIP(hipMemcpy(e->fft_tw.p, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
        }
    }
    if (e->fast && e->taps_cap >= hd_engine::kLpFftMinTaps && getenv("HD_NO_LP_FFT") == nullptr) {     // (HD_NO_LP_FFT=1: long filters as direct sums in fast mode too)
        std::call_once(g_rocfft_once, [] { rocfft_setup(); });
        uint32_t N = 1;
        while (N < m_cap + e->taps_cap) N <<= 1;
        e->lpf_N[1] = N; e->lpf_N[0] = N / 2;
        size_t wmax = 0;
        for (int w = 0; w < 2; ++w) {
            const size_t len = e->lpf_N[w];
            if (rocfft_plan_create(&e->lpf_fwd[w], rocfft_placement_inplace, rocfft_transform_type_complex_forward, rocfft_precision_single, 1, &len, S, nullptr) != rocfft_status_success ||
                rocfft_plan_create(&e->lpf_inv[w], rocfft_placement_inplace, rocfft_transform_type_complex_inverse, rocfft_precision_single, 1, &len, S, nullptr) != rocfft_status_success)
                return fail(HD_ERR_DEVICE, "rocfft_plan_create (low-pass transforms) failed");
            for (rocfft_plan pl : {e->lpf_fwd[w], e->lpf_inv[w]}) { size_t wsz = 0; rocfft_plan_get_work_buffer_size(pl, &wsz); wmax = std::max(wmax, wsz); }
        }
        if (rocfft_execution_info_create(&e->lpf_info) != rocfft_status_success) return fail(HD_ERR_DEVICE, "rocfft_execution_info_create failed");
        if (wmax) { HD_HIP(e->lpf_workbuf.alloc(wmax)); rocfft_execution_info_set_work_buffer(e->lpf_info, e->lpf_workbuf.p, wmax); }
        HD_HIP(e->lpf_x.alloc((size_t)S * N));
        HD_HIP(e->lpf_k.alloc((size_t)S * N));
        HD_HIP(e->lpf_ntaps.alloc(S));
        HD_HIP(e->lpf_flags.alloc((size_t)S * 2));
    }
    // Pay first-use costs now: run every kernel once on an all-idle call.
    {
        hd_engine::CallSlot& sl = e->slot[0];
        hipStream_t q = e->qa;
        const uint32_t T1 = e->stages.size() > 0 ? (uint32_t)e->stages[0].taps.size() : 0, T2 = e->stages.size() > 1 ? (uint32_t)e->stages[1].taps.size() : 0;
        if (e->stages.empty()) HDK(launch_passthrough, q, S, 1, e->staging.p, cfg->max_chunk, e->fbuf[0].p, e->fbuf_stride, sl.d_call.p, e->fir_hist_cap);
        if (e->stages.size() >= 1)
            HDK(launch_decimate, q, e->stages[0].ratio, T1, S, 1, e->staging.p, cfg->max_chunk, e->hist1[0].p, e->hist1[1].p, e->stage_taps[0].p,
                                e->stages.size() == 1 ? e->fbuf[0].p : e->dec1.p, e->stages.size() == 1 ? e->fbuf_stride : e->n1_cap, sl.d_call.p, 0,
                                e->stages.size() == 1, e->fir_hist_cap, nullptr);
        if (e->stages.size() >= 1)      // (the first stage of a front-tuned call; the slot's tuning block is all zeros: no stream is rotated)
            HDK(launch_decimate_tuned, q, e->stages[0].ratio, T1, S, 1, e->staging.p, cfg->max_chunk, e->hist1[0].p, e->hist1[1].p, e->stage_taps[0].p,
                                      e->stages.size() == 1 ? e->fbuf[0].p : e->dec1.p, e->stages.size() == 1 ? e->fbuf_stride : e->n1_cap, sl.d_call.p,
                                      e->stages.size() == 1, e->fir_hist_cap, nullptr, 0u, sl.h_front.dev, e->tune_tab.p);
        if (e->stages.size() == 2)
            HDK(launch_decimate, q, e->stages[1].ratio, T2, S, 1, e->dec1.p, e->n1_cap, e->hist2[0].p, e->hist2[1].p, e->stage_taps[1].p, e->fbuf[0].p,
                                e->fbuf_stride, sl.d_call.p, 1, 1, e->fir_hist_cap, nullptr);
        HDK(launch_chunk_post, q, S, e->fbuf[0].p, e->fbuf_stride, sl.d_call.p, e->fir_hist_cap, nullptr, e->tune_tab.p);
        if (cfg->enable_spectrum) {
            HDK(launch_fft_feed, q, S, e->fbuf[0].p, e->fbuf_stride, e->fft_in.p, sl.d_call.p, e->fir_hist_cap);
            hd::launch_spectrum_wave(q, S, e->fft_in.p, e->fft_tw.p, e->spec.p, e->power.p, sl.h_stats.dev, sl.d_call.p, e->fsd, e->bins_sep, 0u);   // (fft_run = 0 everywhere: every wave returns at once)
        }
        if (!HDK(launch_fir_demod, q, S, 0, 0, e->lds_per_wg, e->fbuf[0].p, e->fbuf_stride, e->lp_taps.p, e->taps_cap, e->demod.p, e->demod.n / S, nullptr, e->carry[0].p,
                             e->carry[1].p, sl.d_call.p, e->fir_hist_cap, e->tail.p, e->tail_cap, e->d_symstate.p, e->fbuf[1].p,
                             e->fir_head.p, e->head_cap, e->fbuf[2].p)) return fail(HD_ERR_DEVICE, "low-pass kernel refused its smallest launch");
        HDK(launch_symbols, q, S, 1, 1, e->max_R, e->tail.p, e->tail_cap, e->d_symstate.p, e->flipmask.p, e->weight.p, e->d_sym.p, sl.d_call.p,
                           sl.h_slots.dev, e->slot_words, nullptr, 0, e->min_R, 0u);
        HD_HIP(hipStreamSynchronize(q));
        HD_HIP(hipGetLastError());        // a kernel this shape cannot launch (LDS, grid) fails the creation, not every later call
        // the all-idle call moved nothing, but the history / carry ping-pong "out" buffers were written: restore zeros
        for (auto& h : e->hist1) if (h.p) HD_HIP(hipMemset(h.p, 0, h.n * sizeof(float2)));
        for (auto& h : e->hist2) if (h.p) HD_HIP(hipMemset(h.p, 0, h.n * sizeof(float2)));
        for (auto& c : e->carry) HD_HIP(hipMemset(c.p, 0, c.n * sizeof(hd::DemodCarry)));
        HD_HIP(hipMemset(e->d_symstate.p, 0, S * sizeof(hd::SymState)));
        if (const char* b0 = getenv("HD_SYM_BASE0")) {
            // test hook: start every stream's monotonic 32-bit sample position somewhere else than 0 (e.g. just below 2^32, which
            // a 32 kHz stream otherwise reaches after 37 hours), to exercise the wrap-around of the symbol rings' positions
            hd::SymState st0{};
            st0.base = st0.cached = st0.run_pos = (uint32_t)strtoul(b0, nullptr, 0);
            std::vector<hd::SymState> v(S, st0);
            HD_HIP(hipMemcpy(e->d_symstate.p, v.data(), S * sizeof(hd::SymState), hipMemcpyHostToDevice));
        }
    }
    HD_HIP(hipDeviceSynchronize());
    *out = e.release();
    return HD_OK;
}

void hd_engine_destroy(hd_engine* e)
{
    if (!e) return;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    delete e;
}

uint32_t hd_engine_streams(const hd_engine* e) { return e ? e->S : 0; }
uint32_t hd_engine_decimation(const hd_engine* e) { return e ? e->D : 0; }
double hd_engine_decimated_rate(const hd_engine* e) { return e ? e->fsd : 0; }
uint32_t hd_engine_lowpass_taps_max(const hd_engine* e) { return e ? std::min(e->taps_cap, e->lp_taps_max) : 0; }
uint64_t hd_engine_sentences_ok(const hd_engine* e) { return e ? e->sentences_ok : 0; }
void hd_engine_set_timing(hd_engine* e, int on) { if (e) e->timing_every = on < 0 ? 0u : (uint32_t)on; }
int hd_engine_timing(hd_engine* e, hd_timing* out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = e->last_timing;
    out->host_calls_in_place = e->host_calls_in_place;
    out->lowpass_fft_calls = e->lpf_calls;
    return HD_OK;
}

// diagnostic (not in include/habdec_amd.h): the two sets of per-XCD run counters of the step launches, [2][16] (after a device-wide wait)
extern "C" int hd_debug_step_counters(hd_engine* e, unsigned int* out32)
{
    if (!e || !out32) return HD_ERR_INVALID;
    std::vector<unsigned int> h(2 * 16 * 32);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), e->step_ctr.p, h.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return HD_ERR_DEVICE;
    for (int i = 0; i < 32; ++i) out32[i] = h[(size_t)i * 32];
    return HD_OK;
}

void hd_set_sentence_callback(hd_engine* e, hd_sentence_cb cb, void* user) { if (e) { e->sentence_cb = cb; e->sentence_user = user; } }
void hd_set_match_callback(hd_engine* e, hd_match_cb cb, void* user) { if (e) { e->match_cb = cb; e->match_user = user; } }
void hd_set_chars_callback(hd_engine* e, hd_chars_cb cb, void* user) { if (e) { e->chars_cb = cb; e->chars_user = user; } }

/* ---------------------------------------------------------------- control plane -------------------------------- */

int hd_stream_set_baud(hd_engine* e, uint32_t s, double baud)
{
    if (int r = check_stream(e, s)) return r;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    if (baud > 0 && e->fsd / baud < 3.5)
        return fail(HD_ERR_UNSUPPORTED, "symbol rate above a third of the decimated rate (fewer than 4 samples per bit): the symbol extractor's windows would overlap");
    StreamHost probe = e->st[s];
    probe.baud = baud;
    const hd::SymbolParams p = symbol_params(e, probe);
    if (p.spb) {
        const uint32_t need = 3u * e->backlog_cap / p.spb + 64u;
        if (need > (e->slot_words - sizeof(hd::BitsHeader) / 4) * 32)
            return fail(HD_ERR_CAPACITY, "baud too high for the result slots sized at engine creation");
        if (p.R > e->max_R) e->max_R = p.R;
        if (p.R < e->min_R) e->min_R = std::max<uint32_t>(p.R, 4);
    }
    e->st[s].baud = baud;
    e->st[s].sym_reset = true;
    e->sym_dirty = true;
    return HD_OK;
}
int hd_stream_set_rtty(hd_engine* e, uint32_t s, uint32_t bits, float stops)
{
    if (int r = check_stream(e, s)) return r;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    e->st[s].text.framer.nbits = bits;
    e->st[s].text.framer.nstops = stops;
    return HD_OK;
}
int hd_stream_set_lowpass_bw(hd_engine* e, uint32_t s, float hz)         // Decoder.h:238-243
{
    if (int r = check_stream(e, s)) return r;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    StreamHost& st = e->st[s];
    st.lp_bw = hz;
    if (st.lp.design(cutoff_rel(e, st), st.lp_trans)) st.taps_dirty = true;
    return HD_OK;
}
int hd_stream_set_lowpass_trans(hd_engine* e, uint32_t s, float trans)   // Decoder.h:252-257
{
    if (int r = check_stream(e, s)) return r;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    StreamHost& st = e->st[s];
    st.lp_trans = trans;
    if (st.lp.design(cutoff_rel(e, st), st.lp_trans)) st.taps_dirty = true;
    return HD_OK;
}
int hd_stream_set_dc_remove(hd_engine* e, uint32_t s, int on)
{
    if (int r = check_stream(e, s)) return r;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    e->st[s].dc = on != 0;
    return HD_OK;
}
int hd_stream_reset_frequency_correction(hd_engine* e, uint32_t s, double c)
{
    if (int r = check_stream(e, s)) return r;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    e->st[s].afc.reset(c, hd::kFftBins, e->fsd);
    return HD_OK;
}
// Tuning: the offset takes effect from the next call submitted; the phase carries on (f = 0 clears it: the stream is untouched again)
int hd_stream_set_tune(hd_engine* e, uint32_t s, double offset_hz)
{
    if (int r = check_stream(e, s)) return r;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    uint32_t d = 0;
    if (!hd::tune_step(offset_hz, e->fsd, &d)) return fail(HD_ERR_INVALID, "tuning offset outside (-fs_dec/2, fs_dec/2)");
    StreamHost& st = e->st[s];
    st.tune_hz = offset_hz; st.tune_step = d; st.tune_from = e->calls;
    if (offset_hz == 0) e->mirror[s].tune_phase = 0;
    return HD_OK;
}
// Tuning at the input rate: same rules, the step in units of the INPUT rate; the phase advances by the call's input samples (plan_call)
int hd_stream_set_front_tune(hd_engine* e, uint32_t s, double offset_hz)
{
    if (int r = check_stream(e, s)) return r;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    if (e->stages.empty()) return fail(HD_ERR_UNSUPPORTED, "an engine without a decimation stage has no input-rate tuning: hd_stream_set_tune is the same thing there");
    uint32_t d = 0;
    if (!hd::tune_step(offset_hz, e->fs, &d)) return fail(HD_ERR_INVALID, "tuning offset outside (-fs/2, fs/2)");
    StreamHost& st = e->st[s];
    st.front_hz = offset_hz; st.front_step = d; st.front_from = e->calls;
    if (offset_hz == 0) e->mirror[s].front_phase = 0;
    return HD_OK;
}
int hd_stream_front_tune(hd_engine* e, uint32_t s, hd_front_tune_info* out)
{
    if (int r = check_stream(e, s)) return r;
    if (!out) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    const StreamHost& st = e->st[s];
    out->offset_hz = st.front_hz; out->step = st.front_step; out->phase = e->mirror[s].front_phase; out->from_call = st.front_from;
    return HD_OK;
}
int hd_stream_set_auto_afc(hd_engine* e, uint32_t s, int on, double hold_s, double min_hz)
{
    if (int r = check_stream(e, s)) return r;
    if (!(hold_s >= 0) || !(min_hz >= 0)) return fail(HD_ERR_INVALID, "hold_s and min_hz must be >= 0");
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    StreamHost& st = e->st[s];
    st.auto_afc = on != 0; st.afc_hold_s = hold_s; st.afc_min_hz = min_hz; st.afc_elapsed = 0;
    return HD_OK;
}
int hd_stream_tune(hd_engine* e, uint32_t s, hd_tune_info* out)
{
    if (int r = check_stream(e, s)) return r;
    if (!out) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    const StreamHost& st = e->st[s];
    out->offset_hz = st.tune_hz; out->step = st.tune_step; out->phase = e->mirror[s].tune_phase;
    out->retunes = st.retunes; out->from_call = st.tune_from; out->auto_afc = st.auto_afc ? 1 : 0;
    return HD_OK;
}

// framing trial (host/format_trial.hpp)
int hd_stream_set_format_trial(hd_engine* e, uint32_t s, int on)
{
    if (check_stream(e, s)) return HD_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    e->st[s].trial.reset(on ? new hd::FormatTrial : nullptr);
    return HD_OK;
}

int hd_stream_format_trial(hd_engine* e, uint32_t s, hd_format_trial_result* out)
{
    if (check_stream(e, s)) return HD_ERR_INVALID;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    if (!e->st[s].trial) return fail(HD_ERR_INVALID, "the stream's framing trial is off (hd_stream_set_format_trial)");
    e->st[s].trial->get(out);
    return HD_OK;
}

}  // extern "C"

/* ---------------------------------------------------------------- data path ------------------------------------ */

namespace {

// Step mode: the tails of the newest call have not been launched yet (they wait for the next call's launch).  Run them now, as a
// kernel of their own -- the next call is not coming (flush), or its results are wanted first.
int run_pending_tail(hd_engine* e)
{
    if (!e->pend.valid) return HD_OK;
    hd_engine::CallSlot& ps = e->slot[e->pend.slot];
    e->pend.valid = false;
    hd::TailArgs ta = e->pend.ta;
    const int lanes = (e->S >= 2 * e->n_cus ? 64 : 256);
    hd::TailArgs lay = ta;
    if (lanes != 64) {      // the pending arguments carry the 64-lane carve of the step launch; a 256-lane kernel needs its own
        // (same buffers, other LDS offsets)
        if (!HDK(tail_layout, lay, lanes, e->pend.r2, e->pend.t2, e->pend_max_taps, e->max_R, e->min_R, e->tail_cap, e->pend.ta.pend_max, 64 * 1024)) return fail(HD_ERR_INVALID, "stream tail layout");
    }
    if (!HDK(launch_tail, e->qa, lanes, e->pend.r2, e->pend.t2, e->S, lay, ps.ev_done)) return fail(HD_ERR_INVALID, "stream tail refused a shape it was selected for");
    HD_HIP(hipGetLastError());
    return HD_OK;
}

// Deliver the results of the call that ran in `sl`: wait for its back half, then the host stages, stream by stream
// (AFC state machine Decoder.h:501-515; RTTY framing, sentence scan, callbacks Decoder.h:559-637).
int collect(hd_engine* e, hd_engine::CallSlot& sl)
{
    if (!sl.busy) return HD_OK;
    if (e->pend.valid && &e->slot[e->pend.slot] == &sl) { if (const int r = run_pending_tail(e)) return r; }
    const auto w0 = std::chrono::steady_clock::now();
    HD_HIP(hipEventSynchronize(sl.ev_done));
    const auto w1 = std::chrono::steady_clock::now();
    sl.busy = false;
    if (sl.timed) {
        float a = 0, b = 0;
        HD_HIP(hipEventElapsedTime(&b, sl.t1, sl.t2));
        if (sl.timed_step) a = b; else HD_HIP(hipEventElapsedTime(&a, sl.t0, sl.t3));
        e->last_timing.ms_total = a;
        e->last_timing.ms_front = b;
        e->last_timing.samples = sl.total_in;
        e->last_timing.front_bytes = sl.total_in * 8 + (sl.total_in / sl.r1) * 8;
        ++e->last_timing.timed_calls;
    }
    int rc = HD_OK;
    {   // every stream's slot must carry this call's tag (the kernels store it last); in practice it is there when the event has fired -- if not, wait for it
        const auto t_lim = std::chrono::steady_clock::now() + std::chrono::milliseconds(200);
        const bool timing_experiment = e->cu_exp != 0;      // (only in the -DHD_TIMING_EXPERIMENT variant build: step launches without their tails or without stage 1 -- nothing writes the slots)
        auto await = [&](const volatile uint32_t* tag, const char* what, uint32_t s) {
            for (uint32_t spins = 0; *tag != sl.seq; ++spins) {
                if (std::chrono::steady_clock::now() > t_lim) {
                    e->device_failed = true;
                    e->fail_cause = std::string(what) + " of stream " + std::to_string(s) + " does not carry its call's tag 200 ms after the completion event";
                    rc = fail(HD_ERR_DEVICE, e->fail_cause + ": the results of this engine are unreliable -- destroy the engine");
                    return;
                }
                if (spins > 64u) std::this_thread::yield();      // (in practice the tag is there when the event has fired)
            }
        };
        for (uint32_t s = 0; s < e->S && !e->device_failed && !timing_experiment; ++s) {
            await(&reinterpret_cast<const volatile hd::BitsHeader*>(sl.h_slots.p + (size_t)s * e->slot_words)->seq, "result slot", s);
            // ... and the spectrum statistics of a stream whose buffer completed in this call: written by the tail itself (behind the same tag) or by a
            // spectrum launch of its own, whose stores no event of this engine fences
            if (!e->device_failed && e->cfg.enable_spectrum && sl.h_stats.p && hd::sc_fft_run(sl.h_call.p[s]))
                await(reinterpret_cast<const volatile uint32_t*>(&sl.h_stats.p[s].seq), "spectrum statistics", s);
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (e->ring_gave_up.p && e->ring_gave_up.p[0] && !e->device_failed) {
        e->device_failed = true;
        e->fail_cause = "k_stage1_cu (loader / consumer waves): a bounded wait ran out inside a launch (word " + std::to_string(e->ring_gave_up.p[0]) + ")";
    }
    if (e->device_failed && rc == HD_OK)         // (a later call of a failed engine: the cause recorded when it failed)
        rc = fail(HD_ERR_DEVICE, e->fail_cause + ": the results of this and of every later call of this engine are unreliable -- destroy the engine");
    if (e->device_failed) {
        // Nothing of this slot is delivered: the launch that gave up left stage-1 output incomplete, so the characters -- possibly CRC-passing
        // sentences -- framed from it would be handed to the callbacks as if they were results.  No AFC step, no framer push, no callbacks, no counters.
        e->last_timing.host_wait_us = std::chrono::duration<double, std::micro>(w1 - w0).count();
        e->last_timing.host_text_us = 0;
        return rc;
    }
    for (uint32_t s = 0; s < e->S; ++s) {
        StreamHost& st = e->st[s];
        const hd::StreamCall& c = sl.h_call.p[s];
        if (hd::sc_fft_run(c)) {
            std::memcpy(&st.stats, &sl.h_stats.p[s], sizeof(st.stats));
            st.have_spectrum = true;
            ++st.spectra;
        }
        const bool past_batch_gate = c.fir_m || c.clear_pending;
        if (past_batch_gate && e->cfg.enable_spectrum) st.afc.step(st.have_spectrum, st.stats, hd::kFftBins, e->fsd);
        // closed loop (hd_stream_set_auto_afc): the server's AFC block (websocketServer/main.cpp:247-263) in sample time, retuning the stream instead of a radio.
        // The new step rides with the parameters of the next call submitted -- no drain.
        st.afc_elapsed += c.n_in;
        if (st.auto_afc && (double)st.afc_elapsed >= st.afc_hold_s * e->fs && std::abs(st.afc.correction) > st.afc_min_hz) {
            const double corr = st.afc.correction;
            uint32_t d = 0;
            if (hd::tune_step(st.tune_hz + corr, e->fsd, &d)) {
                st.tune_hz += corr; st.tune_step = d; st.tune_from = e->calls;
                if (!d) e->mirror[s].tune_phase = 0;
                st.afc.reset(corr, hd::kFftBins, e->fsd);
                st.afc_elapsed = 0;
                ++st.retunes;
            }
        }
        const uint32_t* slot = sl.h_slots.p + (size_t)s * e->slot_words;
        const hd::BitsHeader* hdr = reinterpret_cast<const hd::BitsHeader*>(slot);
        SizeState& sz = e->mirror[s];
        st.held = hdr->held_after;
        sz.inflight_m -= c.fir_m;
        sz.win_ub = hdr->uncached + sz.inflight_m;
        st.last_nbits = hdr->nbits; st.last_nflips = hdr->nflips;
        st.bits_total += hdr->nbits;
        st.demod_ck[0] = hdr->demod_ck[0]; st.demod_ck[1] = hdr->demod_ck[1]; st.demod_ck_n = hdr->demod_n; st.demod_ck_call = e->delivered;
        if (hdr->demod_n != 0xFFFFFFFFu) {
            for (const uint32_t x : {hdr->demod_n, hdr->demod_ck[0], hdr->demod_ck[1]}) st.demod_ck_hash = (st.demod_ck_hash ^ x) * 0x100000001B3ull;
            ++st.demod_ck_calls;
        } else ++st.demod_ck_unknown;
        if (hdr->overflow & 1u) rc = fail(HD_ERR_CAPACITY, "symbol result slot overflow on stream " + std::to_string(s));
        if (hdr->overflow & 2u) ++st.flip_list_full;     // (the search stopped at the flip-list bound and resumes next call: bits arrive a call later)
        const uint32_t* words = slot + sizeof(hd::BitsHeader) / 4;
        st.last_words.assign(words, words + (hdr->nbits + 31) / 32);
        if (!c.fir_m) continue;
        if (hdr->nbits) st.text.framer.push_packed(words, hdr->nbits);
        if (st.trial) st.trial->push_packed(words, hdr->nbits);
        const std::string chars = st.text.run(hdr->nbits != 0, [&](const hd::SentenceMatch& m) {
            ++e->sentences_ok;
            if (e->sentence_cb) { e->in_callback = true; e->sentence_cb(e->sentence_user, s, m.callsign.c_str(), m.data.c_str(), m.crc.c_str()); e->in_callback = false; }
        }, [&](const hd::SentenceMatch& m, bool ok) {
            if (e->match_cb) { e->in_callback = true; e->match_cb(e->match_user, s, m.callsign.c_str(), m.data.c_str(), m.crc.c_str(), ok ? 1 : 0); e->in_callback = false; }
        });
        if (!chars.empty() && e->chars_cb) { e->in_callback = true; e->chars_cb(e->chars_user, s, chars.data(), chars.size()); e->in_callback = false; }
    }
    e->last_timing.host_wait_us = std::chrono::duration<double, std::micro>(w1 - w0).count();
    e->last_timing.host_text_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w1).count();
    return rc;
}

// Deliver the oldest calls until at most `depth` are undelivered.  Every call is counted as delivered; the last error is returned.
int deliver(hd_engine* e, uint64_t depth)
{
    int rc = HD_OK;
    while (e->calls - e->delivered > depth) {           // oldest first
        if (const int r = collect(e, e->slot[e->delivered % hd_engine::kSlots])) rc = r;
        ++e->delivered;
    }
    return rc;
}

}  // namespace

int hd::eng::flush_locked(hd_engine* e)
{
    // step mode: the newest call's tails have not been launched yet -- start them before the host spends time on the older call's text
    if (e->delivered < e->calls) { if (const int r = run_pending_tail(e)) return r; }
    return deliver(e, 0);
}

namespace {

/* One hd_process_device call, in stages:
 *   plan_call    sizes and the reference's bookkeeping: the slot's StreamCall / tuning entries, a summary (CallPlan), the mirror after the call;
 *   route_call   how the call is launched (CallRoute);
 *   enqueue_*    the uploads, then the step launch or the front and back halves;
 *   commit_call  the planned mirror becomes the streams', the slot goes in flight, the buffers turn;
 *   deliver      older calls' results.
 * No collect() runs between plan_call and commit_call: collect() writes the mirror too (inflight_m, win_ub; tune_phase on an automatic retune). */

enum class Route : uint32_t {   // hd_timing.path
    separate = 0,   // stage kernels, k_fir_demod, k_symbols, spectrum launches
    tail = 2,       // stage 1, then the one-wave stream tails (kernels/tail_body.h) as a launch of their own
    step = 3,       // batch mode: this call's stage 1 with the previous call's stream tails in front, one launch (kernels/decimate.hip k_step)
};

struct CallPlan {
    size_t nst = 0;
    uint32_t R1 = 1, R2 = 1, T1 = 0, T2 = 0;
    uint32_t max_in = 0, min_in = 0xFFFFFFFFu, max_n1 = 0, max_n2 = 0, max_m = 0, max_taps = 0, max_new = 0, max_pend = 0;
    uint64_t total_in = 0;
    bool any_fft = false, any_dc = false, any_zero1 = false, any_tune = false, any_lp_restart = false;
    bool any_front = false;      // some stream of the call is tuned at the input rate: its first stage is k_decimate_tuned, a launch of its own
};

struct CallRoute {
    Route route = Route::separate;
    int tail_lanes = 64;
    hd::TailArgs ta{}, ta_step{};            // LDS carves of the stream tails: as a launch of their own / riding in the next call's step launch
    bool lean = false, free_front = false, host_params = false, any_post = false, spectrum_on_qc = false;
    const hd::StreamCall* dcall = nullptr;   // the call's parameters as the kernels read them
    float2* feed = nullptr;                  // the spectrum collection buffer the final stage fills, or null
};

struct CallBufs {   // this call's turn of the rotating buffers
    float2 *fcur, *fnext, *fprev, *d1;   // low-pass buffers of this call, the next one and the previous one; stage-1 output
    int hin, hout, cin, cout;            // stage histories and discriminator carries: read / written
};

CallBufs call_bufs(const hd_engine* e)
{
    CallBufs b;
    b.fcur = e->fbuf[e->cur].p; b.fnext = e->fbuf[(e->cur + 1) % 3].p; b.fprev = e->fbuf[(e->cur + 2) % 3].p;
    b.d1 = (e->calls % 3 == 0) ? e->dec1.p : (e->calls % 3 == 1) ? e->dec1b.p : e->dec1c.p;   // never a buffer a call in flight still reads
    b.hin = e->hist_cur; b.hout = e->hist_cur ^ 1;
    b.cin = e->carry_cur; b.cout = e->carry_cur ^ 1;
    return b;
}

// The host mirror of the reference's size bookkeeping -> one StreamCall per stream.  Writes the slot's host blocks and e->mirror_next, not the streams'
// mirror.  Its one lasting side effect is the control plane's: a low-pass redesign (`redesigned`: the caller drains the pipeline and plans again).
int plan_call(hd_engine* e, hd_engine::CallSlot& sl, const uint32_t* n_per_stream, uint32_t n_uniform, CallPlan& p, bool& redesigned)
{
    p = CallPlan{};
    p.nst = e->stages.size();
    if (p.nst > 0) { p.R1 = e->stages[0].ratio; p.T1 = (uint32_t)e->stages[0].taps.size(); }
    if (p.nst > 1) { p.R2 = e->stages[1].ratio; p.T2 = (uint32_t)e->stages[1].taps.size(); }
    redesigned = false;
    for (uint32_t s = 0; s < e->S; ++s) {
        StreamHost& st = e->st[s];
        SizeState& nx = e->mirror_next[s];
        nx = e->mirror[s];
        hd::StreamCall c{};
        const uint32_t n = n_per_stream ? n_per_stream[s] : n_uniform;
        c.n_in = n;
        c.n1 = n / p.R1;
        c.n2 = c.n1 / p.R2;
        if (n) {   // Decimator::setInput growth rule (Decimator.h:74-79, Q5)
            if (p.nst > 0) { const size_t want = (size_t)n + p.T1 + p.R1; if (nx.stage_buf[0] < want) { nx.stage_buf[0] = want; c.zero_hist1 = 1; } }
            if (p.nst > 1) { const size_t want = (size_t)c.n1 + p.T2 + p.R2; if (nx.stage_buf[1] < want) { nx.stage_buf[1] = want; c.zero_hist2 = 1; } }
        }
        c.dc_remove = st.dc && c.n2;
        sl.h_tune.p[s] = make_uint2(st.tune_step, nx.tune_phase);     // (read by the kernels only when some stream of the call is tuned)
        if (st.tune_step) { p.any_tune = true; nx.tune_phase += c.n2 * st.tune_step; }
        sl.h_front.p[s] = make_uint2(st.front_step, nx.front_phase);
        if (st.front_step | nx.front_phase) { p.any_front = true; nx.front_phase += n * st.front_step; }
        c.pend_before = (uint32_t)nx.pending;
        nx.pending += c.n2;
        // spectrum collection (Decoder.h:467-489)
        c.fft_fill = (uint32_t)nx.fft_fill;
        if (e->cfg.enable_spectrum && n && nx.fft_fill < (size_t)hd::kFftBins && c.n2) {
            c.fft_take = (uint32_t)std::min<size_t>(hd::kFftBins - nx.fft_fill, c.n2);
            nx.fft_fill += c.fft_take;
        }
        c.fft_run = hd::sc_pack_fft_run(0, nx.fft_buf);
        if (e->cfg.enable_spectrum && n && nx.fft_fill >= (size_t)hd::kFftBins) {
            c.fft_run = hd::sc_pack_fft_run(1, nx.fft_buf); nx.fft_fill = 0; p.any_fft = true;
            nx.spec_buf = nx.fft_buf;
            if (e->lazy_spectra) nx.fft_buf ^= 1u;      // the completed buffer stays as it is until the other one has completed
        }
        // batch gate, rate gate, low-pass batch (Decoder.h:492-542)
        const bool past_batch_gate = n && nx.pending >= hd::kFirBatch;
        nx.last_m = 0;
        if (past_batch_gate && !e->decode_enabled) { c.clear_pending = 1; nx.pending = 0; }
        else if (past_batch_gate) {
            const uint32_t m = (uint32_t)(nx.pending - nx.pending % hd::kFirBatch);
            st.lp.batch = m;                                                       // FirFilter::setInput
            if (st.lp.design(cutoff_rel(e, st), st.lp_trans)) {                    // LP_BlackmanHarris, Decoder.h:538 (only when a stream's batch size changes)
                st.taps_dirty = true;
                redesigned = true;
            }
            const uint32_t T = (uint32_t)st.lp.taps.size();
            if (!T) return fail(HD_ERR_UNSUPPORTED, "low-pass transition width leaves no taps (reference filters nothing then)");
            if (T > e->taps_cap) return fail(HD_ERR_CAPACITY, "low-pass tap count exceeds engine capacity");
            // (the LDS image of k_fir_demod and the sixteen bits of fir_taps_prev: refused here, before anything is queued -- the launch could not happen)
            if (T > e->lp_taps_max)
                return fail(HD_ERR_CAPACITY, "low-pass design of " + std::to_string(T) + " taps on stream " + std::to_string(s) + " exceeds hd_engine_lowpass_taps_max = " + std::to_string(e->lp_taps_max));
            if (nx.fir_buf < (size_t)m + T) { nx.fir_buf = (size_t)m + T; c.fir_zero_hist = 1; }   // FirFilter.h:141-147
            c.fir_m = m; c.fir_taps = T;
            // (tap count of the previous run, and where the first samples of that run's input are: in the previous call's buffer if that is where it ran, else aside)
            c.fir_taps_prev = hd::sc_pack_taps_prev(nx.fir_T_run ? nx.fir_T_run : T, nx.head_n, !nx.head_aside && nx.head_call + 1 == e->calls, false);
            nx.fir_T_run = T;
            nx.head_n = std::min<uint32_t>(m, std::min<uint32_t>(e->head_cap, 0x3FFFu)); nx.head_call = e->calls; nx.head_aside = false;
            nx.pending -= m;
            nx.last_m = m;
            p.max_m = std::max(p.max_m, m);
            p.max_taps = std::max(p.max_taps, T);
            p.any_lp_restart |= c.fir_zero_hist != 0;
            // positions whose windows can become computable this call (device: k_sym_avg range), as an upper bound
            const uint32_t pending_windows = st.sym_reset ? std::max(st.held, nx.win_ub) : nx.win_ub;
            p.max_new = std::max(p.max_new, pending_windows + m + 64u);
            nx.inflight_m += m;
            nx.win_ub += m;
        }
        if (!c.fir_m && nx.head_n && !nx.head_aside) {
            // no run in this call: a head that still sits in the previous call's buffer moves aside now (that buffer is rewritten two calls on)
            if (nx.head_call + 1 == e->calls) c.fir_taps_prev = hd::sc_pack_taps_prev(0, nx.head_n, false, true);
            else nx.head_n = 0;          // (cannot happen: the call behind a run either runs or saves)
            nx.head_aside = true;
        }
        c.pend_after = (uint32_t)nx.pending;
        p.max_pend = std::max(p.max_pend, std::max(c.pend_before, c.pend_after));
        nx.last_n2 = c.n2; nx.last_pend_before = c.pend_before; nx.last_buf = e->cur;
        sl.h_call.p[s] = c;
        p.max_in = std::max(p.max_in, n); p.min_in = std::min(p.min_in, n); p.max_n1 = std::max(p.max_n1, c.n1); p.max_n2 = std::max(p.max_n2, c.n2);
        p.any_dc |= c.dc_remove != 0;
        p.any_zero1 |= c.zero_hist1 != 0;
        p.total_in += n;
    }
    sl.total_in = p.total_in;
    sl.r1 = p.R1;
    sl.seq = (uint32_t)(e->calls + 1u);           // (never the tag this slot carried four calls ago)
    if (!sl.seq) sl.seq = 1u;                     // (0 is what a slot holds before its first call: skipped when the counter wraps after 2^32 calls)
    return HD_OK;
}

// How the call is launched.  Host-side only: it rewrites the slot's StreamCall blocks where a spectrum is read in place, and enqueues nothing.
void route_call(hd_engine* e, hd_engine::CallSlot& sl, const CallPlan& p, CallRoute& r)
{
    const uint32_t S = e->S;
    const int R2 = (int)p.R2, T2 = (int)p.T2;
    r = CallRoute{};
    r.tail_lanes = S >= 2 * e->n_cus ? 64 : 256;
    // The stream tail: stage 2 through the symbol extractor as one wave per stream that walks the call in pieces, so neither the call size nor the tap
    // count has to fit an LDS image.  It is the right shape while a call is short: its time grows with the decimated samples per call, and beyond ~2048
    // of them (e.g. /16 with 65536-sample pushes: 4096) the many-workgroup kernels finish a batch sooner (measured: 156 vs 173 GS/s).  It takes no
    // DC-removing call.  (A handful of streams, long calls: the 256-lane tail in pieces of 1024 outputs where its windows fit -- one piece for a 65536-sample
    // push at /64 --, of 256 otherwise.)
    const bool tail = p.nst == 2 && !p.any_dc && !e->no_tail && p.max_n2 <= e->tail_max_n2 &&
                      ((r.tail_lanes == 256 && p.max_n2 >= 512u && HDK(tail_layout, r.ta, r.tail_lanes, R2, T2, p.max_taps, e->max_R, e->min_R, e->tail_cap, p.max_pend, 64 * 1024, 4)) ||
                       HDK(tail_layout, r.ta, r.tail_lanes, R2, T2, p.max_taps, e->max_R, e->min_R, e->tail_cap, p.max_pend, 64 * 1024));
    // Step mode: batch decoding of equally sized pushes through a single-wave first stage -- ONE launch per call, on one queue: this call's stage 1 with
    // the previous call's stream tails in front.  Its tails are laid out for k_step's static slot here; enqueue_step may re-lay them for k_step_cu.
    const uint32_t step_lds = (p.R1 == 32 || p.R1 == 64) ? HDK(step_lds_bytes, (int)p.R1, (int)p.T1) : 0u;
    // (Not a front-tuned call: the rotation at the input rate exists in k_decimate_tuned only, a launch of its own -- such a call takes the tail route
    // or the separate kernels, whatever it would take on a synchronous engine's side of this test, and a step call's pending tails run as for any
    // other change of route.)
    const bool step = tail && !p.any_front && e->cfg.pipeline && !e->one_stream && p.min_in == p.max_in && p.max_in && step_lds &&
                      HDK(tail_layout, r.ta_step, 64, R2, T2, p.max_taps, e->max_R, e->min_R, e->tail_cap, p.max_pend, step_lds);
    r.route = step ? Route::step : tail ? Route::tail : Route::separate;
    // The separate kernels change the decimated chunk after the last stage (DC blocker, rotation of a tuned stream) in a post-pass; the stream tails
    // rotate in their stage-2 store.
    r.any_post = p.any_dc || (p.any_tune && !tail);
    // Cross-queue event waits cost ~18 us each on this platform (kernel trace: stage 1 of call k+1 started 37 us after stage 1 of call k ended, two barrier
    // packets later).  Behind a stream tail the stage-1 queue therefore waits for NOTHING: it reads the call's parameters straight from the mapped host
    // block (32 bytes per workgroup), its output rotates over three buffers (call_bufs), and the parameter fetch for the back half rides in front of the
    // tails on qb.
    r.lean = tail && !e->one_stream;
    // Round 5: the separate kernels of two-stage plans (calls too large for a one-wave tail: /16 and /256 at 4096 decimated samples per call) do not
    // wait either: the parameter copy rides on qa behind stage 1, which reads the mapped host block.  (Kernel trace before: 15-22 us of barrier packets in
    // front of every stage 1, on the queue a step waits for.)  What the wait protected was the low-pass buffer this call's second stage writes: three take
    // turns, and the back half that read it last is call k-3's, which the host has collected.  The known exception is the FirHistory head the back
    // half of call k-2 reads from that buffer (not covered by the rotation).
    r.free_front = !tail && p.nst == 2 && !e->one_stream;
    // One queue and the stream tails behind stage 1 (synchronous delivery): both kernels read the call's parameters from the mapped host block -- one
    // round trip over PCIe at the start of a workgroup instead of a copy kernel in front of stage 1.
    r.host_params = tail && !step && e->one_stream;
    r.dcall = r.host_params ? sl.h_call.dev : sl.d_call.p;
    // Spectrum collection rides in the final stage's epilogue unless the post-pass must change the samples first.
    r.feed = (e->cfg.enable_spectrum && !r.any_post) ? e->fft_in.p : nullptr;
    if (r.route != Route::separate || !e->cfg.enable_spectrum || r.any_post || !p.any_fft) return;
    // A call whose decimated chunk alone fills a stream's (empty) spectrum buffer: the spectrum launch reads the chunk's head in place and nothing is copied
    // into the collection buffer (fft_take = 0 for the stage that would have fed it; fft_run = 2 for the spectrum kernel) -- at 4096 and more decimated
    // samples per call that is every call: 8 + 8 bytes per decimated sample less traffic.
    for (uint32_t s = 0; s < S; ++s) {
        hd::StreamCall& c = sl.h_call.p[s];
        if (hd::sc_fft_run(c) == 1 && c.fft_fill == 0 && c.fft_take == (uint32_t)hd::kFftBins) { c.fft_take = 0; c.fft_run = hd::sc_pack_fft_run(2, hd::sc_fft_buf(c)); }
    }
    // Where every spectrum of the call is read in place (fft_run == 2 for all of them), the spectrum launch hangs on nothing but this call's chunk: it goes
    // to the third queue behind the front half's event, off the queue a step waits for (round 5 could not: the next call's second stage refilled the
    // collection buffer a transform on another queue was still reading -- there is no collection buffer on this route).
    r.spectrum_on_qc = !e->one_stream && p.nst != 0;
    for (uint32_t s = 0; s < S && r.spectrum_on_qc; ++s) r.spectrum_on_qc = hd::sc_fft_run(sl.h_call.p[s]) != 1u;
}

// Batch mode: a stream tail does not store the call's discriminator output into `demod` -- the same samples are the newest fir_m of the symbol ring it
// appends to, and only hd_stream_demodulated asks for them, behind a flush (4 bytes per decimated sample and launch less, half the stores of the tail's
// discriminator phase).  A synchronous engine keeps the array; so do the separate kernels, where k_symbols reads it.
bool demod_in_ring(const hd_engine* e, Route route) { return e->cfg.pipeline >= 1 && route != Route::separate; }

// Buffers of THIS call's stream tails (the LDS carve is already in t)
void fill_tail(const hd_engine* e, const hd_engine::CallSlot& sl, const CallPlan& p, const CallRoute& r, const CallBufs& b, hd::TailArgs& t)
{
    t.dec1 = b.d1; t.dec1_stride = e->n1_cap; t.hist2_in = e->hist2[b.hin].p; t.hist2_out = e->hist2[b.hout].p; t.taps2 = e->stage_taps[1].p;
    t.fbuf = b.fcur; t.fbuf_next = b.fnext; t.fbuf_stride = e->fbuf_stride; t.fir_hist_cap = e->fir_hist_cap;
    t.lp_taps = e->lp_taps.p; t.taps_stride = e->taps_cap; t.demod = demod_in_ring(e, r.route) ? nullptr : e->demod.p; t.demod_stride = e->demod.n / e->S;
    t.filtered = e->cfg.keep_filtered ? e->filtered.p : nullptr; t.carry_in = e->carry[b.cin].p; t.carry_out = e->carry[b.cout].p;
    t.tune = p.any_tune ? sl.h_tune.dev : nullptr; t.tune_tab = e->tune_tab.p;
    t.call = r.dcall; t.fft_in = r.feed; t.head_buf = e->fir_head.p; t.fbuf_prev = b.fprev; t.head_cap = e->head_cap;
    t.n_streams = e->S;
    t.ring = e->tail.p; t.ring_cap = e->tail_cap; t.sym = e->d_symstate.p; t.flipmask = e->flipmask.p; t.wsum = e->weight.p;
    t.sp = e->d_sym.p; t.slots = sl.h_slots.dev; t.slot_words = e->slot_words; t.seq = sl.seq;
    t.flips_dbg = e->flips_cap ? e->flips_dbg.p : nullptr; t.flips_cap = e->flips_cap;
    t.fft_tw = r.feed ? e->fft_tw.p : nullptr;   // the tail transforms a completed buffer itself (a tail route feeds the buffer exactly when the engine has spectra)
    t.spec = e->lazy_spectra ? nullptr : e->spec.p; t.power = e->lazy_spectra ? nullptr : e->power.p; t.stats = sl.h_stats.dev; t.rate = e->fsd; t.bins_sep = e->bins_sep;
}

// Equally sized pushes through a single-wave first stage of a two-stage plan: the stage-1 workgroups (eight resident per CU) draw runs of tiles from
// per-XCD counters (kernels/decimate.hip) -- no cold start per run, no fixed shares that end ragged.  An empty claim where the shape does not allow it.
// The caller advances e->step_launches once a launch that draws is enqueued (the two counter sets alternate per such launch).
hd::StepClaim make_claim(const hd_engine* e, const CallPlan& p, uint32_t run_len_cu /* != 0: runs for a per-CU ring kernel's loaders */)
{
    hd::StepClaim claim{};
    const int R1 = (int)p.R1, T1 = (int)p.T1;
    const uint64_t S = e->S;
    // (tiles: 64 outputs of a single-wave /32 or /64 first stage; for the per-CU ring kernels hd::ring_tiles -- 64 rows of 32 samples advancing by 57 or 58 at /32, 2048 input samples at the smaller ratios)
    const uint32_t ntiles = run_len_cu ? HDK(ring_tiles, R1, T1, p.max_in) : (p.max_n1 + 63) / 64, n_xcd = e->n_cus / 32u, run_len = run_len_cu ? run_len_cu : e->step_run >= 2 ? e->step_run : 4u;   // (a run must hold the tile in front of which the next draw is issued: at least two; four re-read fewer halos than two)
    const uint64_t runs = S * ntiles / run_len;
    const bool shape_ok = run_len_cu ? (HDK(stage1_cu_supported, R1, T1) && p.max_in % 2048u == 0) : ((R1 == 32 || R1 == 64) && p.max_n1 % 64 == 0);
    if (!e->no_claim && (p.nst == 2 || (run_len_cu && p.nst == 1)) && shape_ok && p.min_in == p.max_in && p.max_in && !p.any_zero1 && n_xcd && e->n_cus % 32u == 0 && n_xcd <= 16 &&
        ntiles && (ntiles % run_len == 0 || (run_len_cu && R1 >= 32 && (S * ntiles) % run_len == 0)) && runs % n_xcd == 0 && S * ntiles < (1ull << 32)) {
        claim.ctr = e->step_ctr.p + (size_t)(e->step_launches & 1u) * 16 * 32;
        claim.ctr_next = e->step_ctr.p + (size_t)((e->step_launches & 1u) ^ 1u) * 16 * 32;
        claim.n_xcd = n_xcd; claim.runs_per_xcd = (uint32_t)(runs / n_xcd); claim.run_len = run_len;
        if (run_len_cu && R1 >= 32 && e->ring_short_pct) {
            // the worker waves' guided hand-out (stage1_ring.h): the last ring_short_pct per cent of an XCD's tiles go out as single tiles
            const uint32_t tpx = claim.runs_per_xcd * run_len, whole = (uint32_t)((uint64_t)tpx * (100u - e->ring_short_pct) / 100u) / run_len;
            claim.tiles_per_xcd = tpx; claim.short_from = whole; claim.runs_per_xcd = whole + (tpx - whole * run_len);
        }
        // Chained tiles (host/ring_schedule.hpp; the /32 worker waves): a ticket is a run of ONE stream, so the ticket space is restated per stream -- the
        // streams must divide among the XCDs, nothing else: runs need not divide anything, a stream's closing run is a ticket like any other.  Of an XCD's
        // share the last ring_short_pct per cent of the STREAMS keep the plain schedule and go out tile by tile behind the chained runs (the guided hand-out;
        // 0: every stream chained, 100: none).  Where the streams do not divide, or a push holds a single tile's rows, the plain grid above stays.
        // (The share: a plain stream costs 36 tiles where a chained one costs 33, so the guided end is bought with tiles; an eighth of the streams measured
        // best on two boxes -- 0.1323 ms per step against 0.1332 with none and 0.1333 with a quarter, NOTES.md -- and is what a launch takes unless told.)
        if (run_len_cu && R1 == 32 && e->ring_chain && S % n_xcd == 0) {
            const uint32_t hr = (uint32_t)((T1 - 1 + 31) / 32), rows = p.max_in / 32u, rl = e->ring_run >= 2u ? e->ring_run : 4u, sx = (uint32_t)(S / n_xcd);
            const hd::RingSchedule ch = hd::ring_schedule(rows, hr, rl, true), pl = hd::ring_schedule(rows, hr, 1u, false);
            const uint32_t sp = hd::ring_plain_streams(sx, e->ring_short_set ? e->ring_short_pct : 12u);
            if (ch.chained && pl.ntiles && (uint64_t)sx * pl.ntiles < (1ull << 31)) {
                claim.chain_rl = ch.rl; claim.chain_sx = sx; claim.chain_sc = sx - sp;
                claim.chain_nfull = ch.n_full; claim.chain_kclose = ch.k_close; claim.chain_ntp = pl.ntiles;
                claim.runs_per_xcd = hd::ring_tickets(ch, pl, sx, sx - sp);
                claim.run_len = ch.rl; claim.short_from = 0xFFFFFFFFu; claim.tiles_per_xcd = 0;
            }
        }
    }
    return claim;
}

// Tiles per drawn run of the per-CU ring kernels: consecutive tiles of one stream (the rows neighbouring tiles share are re-read from the XCD's L2), so it
// must divide the stream's tile count, and the launch's runs must divide among the XCDs.  The /32 stages' worker waves draw their own runs and the
// last runs of a launch are its ragged end: four measured best among 3 / 4 / 6 / 9 / 12 (0.1360-0.1368 ms per step against 0.1386 with nine, one box,
// alternating); the loader / consumer kernels of the smaller ratios keep eight (round 4).  The nearest usable length, the longer one first.
uint32_t pick_ring_run(const hd_engine* e, uint32_t R1, uint32_t ntiles)
{
    const uint64_t S = e->S;
    const uint32_t n_xcd = e->n_cus / 32u ? e->n_cus / 32u : 1u, want = R1 >= 32 ? 4u : 8u;
    // (the worker waves of the /32 and /64 stages walk a run on into the next stream: it need not divide a stream's tiles, only the slab's)
    auto ok = [&](uint32_t r) { return r >= 2u && r <= ntiles && (R1 >= 32 ? (S * ntiles) % r == 0 : ntiles % r == 0) && (S * ntiles / r) % n_xcd == 0; };
    if (e->ring_run >= 2 && ok(e->ring_run)) return e->ring_run;
    for (uint32_t d = 0; d <= 8u; ++d) {
        if (ok(want + d)) return want + d;
        if (d && d < want && ok(want - d)) return want - d;
    }
    return 2u;                                     // (k_step treats shorter runs as "not drawn" while the counter sets have already alternated; make_claim refuses what does not divide)
}

// Everything of the call in front of its first launch: a drain where the route changes, the wait on call k-2, the parameter fetch, the changed tables.
int enqueue_uploads(hd_engine* e, hd_engine::CallSlot& sl, const CallRoute& r)
{
    const uint32_t S = e->S;
    hipStream_t qa = e->qa;
    if (e->last_route >= 0 && e->last_route != (int)r.route) {   // route switch: drain (a pending tail first)
        if (const int rc = run_pending_tail(e)) return rc;
        HD_HIP(hipStreamSynchronize(qa)); HD_HIP(hipStreamSynchronize(e->qb));
    }
    e->last_route = (int)r.route;
    e->last_timing.path = (uint32_t)r.route;
    // (pipelined single-stage plans: the front half writes the low-pass buffer the back half of call k-2 may still be reading)
    if (!r.lean && !r.free_front && e->calls >= 2 && !e->one_stream) HD_HIP(hipStreamWaitEvent(qa, e->slot[(e->calls - 2) % hd_engine::kSlots].ev_done, 0));
    const bool step = r.route == Route::step;
    sl.timed = e->timing_every && (e->calls % e->timing_every) == 0;
    sl.timed_step = sl.timed && step;                       // a step call is ONE launch: two event records (each a barrier packet), not four
    if (sl.timed && !step) HD_HIP(hipEventRecord(sl.t0, qa));
    if (!r.lean && !r.free_front && !r.host_params) {
        // the parameter block is pulled on its own queue, so it does not wait for the previous call's stage 1 to drain
        HDK(launch_fetch_params, e->qc, sl.h_call.dev, sl.d_call.p, S * sizeof(hd::StreamCall));
        if (!e->one_stream) { HD_HIP(hipEventRecord(sl.ev_params, e->qc)); HD_HIP(hipStreamWaitEvent(qa, sl.ev_params, 0)); }
    }
    // (nothing in flight reads the tables uploaded here: a changed table drained the pipeline before the call was planned)
    for (uint32_t s = 0; s < S; ++s) {
        StreamHost& st = e->st[s];
        if (!st.taps_dirty) continue;
        HD_HIP(hipMemcpyAsync(e->lp_taps.p + (size_t)s * e->taps_cap, st.lp.taps.data(), st.lp.taps.size() * 4, hipMemcpyHostToDevice, qa));
        st.taps_dirty = false;
        e->lpf_k_stale = true;
    }
    if (e->sym_dirty) {
        uint32_t mr = 4;
        for (uint32_t s = 0; s < S; ++s) {
            e->h_sym.p[s] = symbol_params(e, e->st[s]);
            e->h_sym.p[s].reset = e->st[s].sym_reset ? 1u : 0u;
            mr = std::max(mr, e->h_sym.p[s].R);
        }
        e->max_R = mr;
        { uint32_t lo = mr; for (uint32_t s2 = 0; s2 < S; ++s2) lo = std::min(lo, std::max<uint32_t>(e->h_sym.p[s2].R, 4)); e->min_R = lo; }
        HD_HIP(hipMemcpyAsync(e->d_sym.p, e->h_sym.p, S * sizeof(hd::SymbolParams), hipMemcpyHostToDevice, qa));
        e->sym_dirty = false;
        for (uint32_t s = 0; s < S; ++s)       // a reset flag is consumed by exactly one call: upload again without it next time
            if (e->st[s].sym_reset) { e->st[s].sym_reset = false; e->sym_dirty = true; }
    }
    return HD_OK;
}

// Step route: ONE launch, [tails of the previous call | this call's stage 1].  Stage 1 reads its parameters from the mapped host block and leaves the
// device copy the tails (next launch) read.  This call's tails are left in r.ta_step for commit_call.
int enqueue_step(hd_engine* e, hd_engine::CallSlot& sl, const CallPlan& p, CallRoute& r, const float2* iq, size_t stride)
{
    const uint32_t S = e->S;
    const int R1 = (int)p.R1, T1 = (int)p.T1, R2 = (int)p.R2, T2 = (int)p.T2;
    hipStream_t qa = e->qa;
    const CallBufs b = call_bufs(e);
    // Where the per-CU step kernel can serve the plan and the sizes, this call's tails are laid out for ITS slice of LDS -- a quarter of what four
    // worker slots leave of the CU's 160 KB (23 KB: larger caches for the search phase than the 20 KB slot of the single-wave fallback) -- now, behind
    // the symbol-table upload; the launch that runs them decides.
    // (... and only where the per-CU kernel's runs can be drawn at all for this stream count -- an odd count never divides among the XCDs --: such
    // batches keep the 20 KB layout and ride in k_step as before.  What is left for the fallback further down are the transitions: a launch that cannot
    // be the per-CU kernel although the previous call expected it.)
    const uint32_t ring_nt = HDK(ring_tiles, R1, T1, p.max_in), ring_run = pick_ring_run(e, p.R1, ring_nt), n_xcd = e->n_cus / 32u;
    const bool runs_ok = ring_nt && n_xcd && ring_run >= 2u && ((uint64_t)S * ring_nt) % ring_run == 0 && ((uint64_t)S * ring_nt / ring_run) % n_xcd == 0;
    const bool cu_shape = !e->no_cu_step && !e->no_claim && !p.any_zero1 && p.max_in % 2048u == 0 && runs_ok && HDK(step_cu_supported, R1, T1, R2, T2);
    const uint32_t cu_tail = cu_shape ? HDK(step_cu_tail_lds, R1, T1) : 0u;
    if (cu_tail) {
        hd::TailArgs tacu{};
        if (HDK(tail_layout, tacu, 64, R2, T2, p.max_taps, e->max_R, e->min_R, e->tail_cap, p.max_pend, cu_tail)) r.ta_step = tacu;
    }
    fill_tail(e, sl, p, r, b, r.ta_step);
    hd_engine::PendingTail prev = e->pend;
    hd_engine::CallSlot* ps = prev.valid ? &e->slot[prev.slot] : nullptr;
    // Events of a k_step_cu launch ride on its dispatch packet (launch_step_cu): t1 / t2 when the call is timed, the previous call's ev_done otherwise.  An
    // event recorded behind a launch is a barrier packet of its own and costs the queue ~5 us before the next launch starts: only a timed launch and the
    // single-wave fallback record ev_done that way.
    const int cu_exp = e->cu_exp;             // timing experiments only (results wrong): 1 = no tails, 2 = no stage 1
    // One workgroup per CU (four stage-1 worker waves, the tails in the other four) where the plan and the sizes allow it
    const bool want_cu = cu_tail && ((cu_exp & 1) || (r.ta_step.lds_bytes <= cu_tail && (!prev.valid || prev.ta.lds_bytes <= cu_tail)));
    const hd::StepClaim claim = make_claim(e, p, want_cu ? ring_run : 0u);
    bool launched = false;
    if (want_cu && claim.ctr) {
        const uint32_t tb = std::max(r.ta_step.lds_bytes, prev.valid ? prev.ta.lds_bytes : 0u);
        hd::StepClaim cl = claim;
        if (cu_exp & 2) { cl.runs_per_xcd = 0; cl.tiles_per_xcd = 0; cl.short_from = 0xFFFFFFFFu; }
        launched = HDK(launch_step_cu, qa, R1, T1, prev.valid ? prev.r2 : R2, prev.valid ? prev.t2 : T2, S, e->n_cus, iq, stride,
                                      e->hist1[b.hin].p, e->hist1[b.hout].p, e->stage_taps[0].p, b.d1, e->n1_cap, sl.h_call.dev, sl.d_call.p, prev.ta,
                                      (prev.valid && !(cu_exp & 1)) ? S : 0u, p.max_in, cl, tb,
                                      sl.timed ? sl.t1 : nullptr, sl.timed ? sl.t2 : ps ? ps->ev_done : nullptr);
    }
    e->last_timing.step_variant = launched ? 1u : 0u;
    if (launched) ++e->step_launches;
    else {
        if (sl.timed) HD_HIP(hipEventRecord(sl.t1, qa));
        // (runs cut for the ring kernel's tiles are not k_step's: fixed shares, and the counter set is not drawn from; drawn runs are short, fixed
        // shares are not: the dispatcher evens out the tail of the launch)
        const hd::StepClaim fb = (want_cu && claim.ctr) ? hd::StepClaim{} : claim;
        const uint32_t wgs = (fb.ctr ? 8u : 32u) * e->n_cus;
        // The previous call's tails were laid out when THAT call was enqueued -- for k_step_cu's 23 KB slice where its shape held -- and the launch that runs
        // them is this one.  If this launch is the single-wave fallback (the pushes grew, a stream count whose runs do not divide among the XCDs, a size
        // that is not a multiple of 2048), a tail carved for more than k_step's static slot would read and write LDS past the workgroup's allocation
        // (reads return 0, writes are dropped: wrong window sums and flips, no error -- ADVICE r05).  Such tails run as a launch of their own, in front,
        // with the LDS they were laid out for; this launch then carries stage 1 only.
        if (prev.valid && prev.ta.lds_bytes > HDK(step_lds_bytes, R1, T1)) {
            if (const int rc = run_pending_tail(e)) return rc;     // (e->pend is still the previous call's; its ev_done rides on that launch)
            prev.valid = false; ps = nullptr;
        }
        if (!HDK(launch_step, qa, R1, T1, prev.valid ? prev.r2 : R2, prev.valid ? prev.t2 : T2, S, p.max_n1, iq, stride, e->hist1[b.hin].p,
                             e->hist1[b.hout].p, e->stage_taps[0].p, b.d1, e->n1_cap, sl.h_call.dev, sl.d_call.p, wgs, prev.ta, prev.valid ? S : 0u,
                             p.any_zero1 ? 0u : p.max_in, fb))
            return fail(HD_ERR_INVALID, "no step kernel for this decimation plan");
        if (fb.ctr) ++e->step_launches;
    }
    if (sl.timed && !launched) HD_HIP(hipEventRecord(sl.t2, qa));
    if (ps && (!launched || sl.timed)) HD_HIP(hipEventRecord(ps->ev_done, qa));    // (a timed launch's own signal is its t2)
    HD_HIP(hipGetLastError());
    return HD_OK;
}

// The spectrum of the streams whose 4096-sample buffer completed in this call (Decoder.h:475-489) as a launch of its own, one wave per stream
// (kernels/spectrum_wave.hip): the separate-kernels route only -- a stream tail transforms its stream's buffer itself.
void call_spectrum(hd_engine* e, hipStream_t q, hd_engine::CallSlot& sl, const CallPlan& p, const CallRoute& r)
{
    if (!(e->cfg.enable_spectrum && p.max_n2)) return;
    const float2* fcur = e->fbuf[e->cur].p;
    if (r.any_post || p.nst == 0) HDK(launch_fft_feed, q, e->S, fcur, e->fbuf_stride, e->fft_in.p, r.dcall, e->fir_hist_cap);
    if (!p.any_fft) return;   // (every call at >= 4096 decimated samples per push)
    hd::launch_spectrum_wave(q, e->S, e->fft_in.p, e->fft_tw.p, e->spec.p, e->power.p, sl.h_stats.dev, r.dcall, e->fsd, e->bins_sep, sl.seq, fcur, e->fbuf_stride, e->fir_hist_cap);
}

// Front half on qa (routes 0 and 2): decimation, [post-pass, spectrum]
int enqueue_front(hd_engine* e, hd_engine::CallSlot& sl, const CallPlan& p, const CallRoute& r, const float2* iq, size_t stride)
{
    const uint32_t S = e->S, R1 = p.R1, T1 = p.T1;
    const bool tail = r.route == Route::tail;
    hipStream_t qa = e->qa;
    const CallBufs b = call_bufs(e);
    if (p.nst == 0) {
        if (sl.timed) HD_HIP(hipEventRecord(sl.t1, qa));
        HDK(launch_passthrough, qa, S, p.max_in, iq, stride, b.fcur, e->fbuf_stride, r.dcall, e->fir_hist_cap);
        if (sl.timed) HD_HIP(hipEventRecord(sl.t2, qa));
    } else {
        const bool single = p.nst == 1;
        float2* out1 = single ? b.fcur : b.d1;
        const size_t out1_stride = single ? e->fbuf_stride : e->n1_cap;
        // (a /64 workgroup holds 36.7 KB of LDS and ~400 VGPRs: four fit a CU, and six per CU would be a launch of one round and a half --
        // measured at 10 MS/s, /256: 1.73 against 1.84 ms per step)
        const uint32_t wgs_cu = (R1 == 64 && !e->dec_wgs_forced && e->dec_wgs_per_cu > 4u) ? 4u : e->dec_wgs_per_cu;
        const uint32_t lin1 = (p.min_in == p.max_in && p.max_in) ? wgs_cu * e->n_cus : 0u;
        // A /32 first stage over equally sized pushes: one workgroup per CU, LDS-DMA loader waves + computing waves (k_stage1_cu, stage1_ring.h)
        bool s1_cu = false;
        if (!p.any_front && (single ? R1 == 4 : R1 != 4) && p.min_in == p.max_in && p.max_in && !e->no_cu_step && !p.any_zero1 && p.max_in % 2048u == 0 && HDK(stage1_cu_supported, (int)R1, (int)T1)) {
            const hd::StepClaim cl = make_claim(e, p, pick_ring_run(e, R1, HDK(ring_tiles, (int)R1, (int)T1, p.max_in)));
            if (cl.ctr) {
                if (sl.timed) HD_HIP(hipEventRecord(sl.t1, qa));
                s1_cu = HDK(launch_stage1_cu, qa, (int)R1, (int)T1, e->n_cus, iq, stride, e->hist1[b.hin].p, e->hist1[b.hout].p, e->stage_taps[0].p, out1, out1_stride,
                                             p.max_in, cl, e->ring_gave_up.dev, (e->cfg.pipeline && !tail && !single) ? hd_engine::kS1Slots : 8u,   // (/4 as the only stage is bound by the vector pipes: eight slots, 0.838 against 0.904 ms per step with four)
                                             single ? r.dcall : nullptr, e->fir_hist_cap, single ? r.feed : nullptr);
                if (s1_cu) ++e->step_launches;
            }
        }
        e->last_timing.step_variant = s1_cu ? 1u : 0u;
        if (!s1_cu) {
            // (stage 1 alone is HBM-bound: drawing runs there cost 3 % -- more halo re-reads -- where the step launch gains 4 %: fixed shares)
            if (sl.timed) HD_HIP(hipEventRecord(sl.t1, qa));
            const hd::StreamCall* call1 = (r.lean || r.free_front) ? sl.h_call.dev : r.dcall;
            if (!(p.any_front ? HDK(launch_decimate_tuned, qa, R1, T1, S, p.max_n1, iq, stride, e->hist1[b.hin].p, e->hist1[b.hout].p, e->stage_taps[0].p, out1, out1_stride,
                                                          call1, single ? 1 : 0, e->fir_hist_cap, single ? r.feed : nullptr, lin1, sl.h_front.dev, e->tune_tab.p)
                              : HDK(launch_decimate, qa, R1, T1, S, p.max_n1, iq, stride, e->hist1[b.hin].p, e->hist1[b.hout].p, e->stage_taps[0].p, out1, out1_stride,
                                                    call1, 0, single ? 1 : 0, e->fir_hist_cap, single ? r.feed : nullptr, lin1)))
                return fail(HD_ERR_INVALID, "no kernel for this decimation stage");
        }
        if (sl.timed) HD_HIP(hipEventRecord(sl.t2, qa));
        if (r.free_front) HDK(launch_fetch_params, qa, sl.h_call.dev, sl.d_call.p, S * sizeof(hd::StreamCall));
        if (!single && !tail) {
            // (Round 4 measured the second stage as a ring kernel too -- /2 with sixteen outputs per lane, /4 with eight: bit-identical, and SLOWER in the
            // pipelined step (/16: 0.338-0.342 against 0.326-0.338 ms): a ring kernel takes a CU's whole LDS, and the back half of the previous call
            // can no longer share the CU with it.  The classic grid stays.  NOTES.md.)
            if (!HDK(launch_decimate, qa, p.R2, p.T2, S, p.max_n2, b.d1, e->n1_cap, e->hist2[b.hin].p, e->hist2[b.hout].p, e->stage_taps[1].p, b.fcur,
                                     e->fbuf_stride, r.dcall, 1, 1, e->fir_hist_cap, r.feed))
                return fail(HD_ERR_INVALID, "no kernel for this decimation stage");
        }
    }
    if (!tail) {
        if (r.any_post) HDK(launch_chunk_post, qa, S, b.fcur, e->fbuf_stride, r.dcall, e->fir_hist_cap, p.any_tune ? sl.h_tune.dev : nullptr, e->tune_tab.p);
        if (!r.spectrum_on_qc) call_spectrum(e, qa, sl, p, r);
    }
    if (!e->one_stream) HD_HIP(hipEventRecord(sl.ev_front, qa));
    if (r.spectrum_on_qc) {
        HD_HIP(hipStreamWaitEvent(e->qc, sl.ev_front, 0));
        call_spectrum(e, e->qc, sl, p, r);
        HD_HIP(hipEventRecord(sl.ev_spec, e->qc));
    }
    return HD_OK;
}

// Fast mode, a long low-pass (configs[4]: 4097 taps): filter through transforms -- [history | inputs | zeros] of N per stream, X conj(K), back -- so that
// k_fir_demod is handed the filtered samples (it still does the discriminator, the ring append, the carries, the slide).  Returns the transform length in
// *lpN, 0 where the direct sums run.
int lowpass_transforms(hd_engine* e, const CallPlan& p, const CallRoute& r, const CallBufs& b, const uint32_t tag, uint32_t* lpN)
{
    *lpN = 0;
    // (Not the run that starts a stream's filter from zeros: a transform's rounding is ~1e-6 of the input's PEAK everywhere, and the start-up transient -- outputs
    // that are exactly zero or tiny in the direct sum -- would come out as noise at that floor, which the discriminator turns into arbitrary phases.)
    if (!e->fast || !e->lpf_N[1] || p.max_taps < hd_engine::kLpFftMinTaps || !p.max_m || p.any_lp_restart) return HD_OK;
    const uint32_t S = e->S, Lmax = p.max_m + p.max_taps - 1;
    const int w = Lmax <= e->lpf_N[0] ? 0 : Lmax <= e->lpf_N[1] ? 1 : -1;
    if (w < 0) return HD_OK;
    const uint32_t N = e->lpf_N[w];
    hipStream_t qb = e->qb;
    rocfft_execution_info_set_stream(e->lpf_info, qb);
    if (e->lpf_k_stale || e->lpf_k_N != N) {           // the taps' spectra, once per design and transform length (a design change has drained the pipeline)
        for (uint32_t s = 0; s < S; ++s) e->lpf_ntaps.p[s] = (uint32_t)e->st[s].lp.taps.size();
        HDK(launch_lp_taps_gather, qb, S, e->lp_taps.p, e->taps_cap, e->lpf_ntaps.dev, e->lpf_k.p, N);
        void* kb[1] = {e->lpf_k.p};
        if (rocfft_execute(e->lpf_fwd[w], kb, nullptr, e->lpf_info) != rocfft_status_success) return fail(HD_ERR_DEVICE, "rocfft_execute (low-pass taps) failed");
        e->lpf_k_N = N; e->lpf_k_stale = false;
    }
    HDK(launch_lp_gather, qb, S, b.fcur, e->fbuf_stride, e->lpf_x.p, N, r.dcall, e->fir_hist_cap, e->fir_head.p, e->head_cap, b.fprev, e->lpf_flags.p, tag);
    void* xb[1] = {e->lpf_x.p};
    if (rocfft_execute(e->lpf_fwd[w], xb, nullptr, e->lpf_info) != rocfft_status_success) return fail(HD_ERR_DEVICE, "rocfft_execute (low-pass forward) failed");
    HDK(launch_lp_mul, qb, S, e->lpf_x.p, e->lpf_k.p, N, r.dcall);
    if (rocfft_execute(e->lpf_inv[w], xb, nullptr, e->lpf_info) != rocfft_status_success) return fail(HD_ERR_DEVICE, "rocfft_execute (low-pass inverse) failed");
    ++e->lpf_calls;
    *lpN = N;
    return HD_OK;
}

// Back half on qb (routes 0 and 2): [stage 2 +] low-pass + discriminator + buffer slide, [spectrum,] symbol extractor, results.  It may still be running
// when the NEXT call's front half starts on qa: the two halves touch disjoint buffers (DESIGN.md "two-stream pipeline").
int enqueue_back(hd_engine* e, hd_engine::CallSlot& sl, const CallPlan& p, CallRoute& r)
{
    const uint32_t S = e->S;
    hipStream_t qb = e->qb;
    const CallBufs b = call_bufs(e);
    if (!e->one_stream) HD_HIP(hipStreamWaitEvent(qb, sl.ev_front, 0));
    // the call's completion event rides on the dispatch of the back half's last launch
    const bool ev_ride = !sl.timed && e->one_stream;   // (two queues: the event is not on the step's critical path, and /16 measured no better with it on the dispatch)
    if (r.route == Route::tail) {
        if (r.lean) HDK(launch_fetch_params, qb, sl.h_call.dev, sl.d_call.p, S * sizeof(hd::StreamCall));
        fill_tail(e, sl, p, r, b, r.ta);
        if (!HDK(launch_tail, qb, r.tail_lanes, (int)p.R2, (int)p.T2, S, r.ta, ev_ride ? sl.ev_done : nullptr)) return fail(HD_ERR_INVALID, "stream tail refused a shape it was selected for");
    } else {
        uint32_t lpN = 0;
        if (const int rc = lowpass_transforms(e, p, r, b, sl.seq, &lpN)) return rc;
        if (!HDK(launch_fir_demod, qb, S, p.max_m, lpN ? 0u : p.max_taps, e->lds_per_wg, b.fcur, e->fbuf_stride, e->lp_taps.p, e->taps_cap, e->demod.p, e->demod.n / S,
                             e->cfg.keep_filtered ? e->filtered.p : nullptr, e->carry[b.cin].p, e->carry[b.cout].p, r.dcall, e->fir_hist_cap,
                             e->tail.p, e->tail_cap, e->d_symstate.p, b.fnext, e->fir_head.p, e->head_cap, b.fprev, e->demod_ck_acc.p,
                             lpN ? e->lpf_x.p : nullptr, lpN, lpN ? 1.0f / (float)lpN : 1.0f, lpN ? e->lpf_flags.p : nullptr, sl.seq))
            return fail(HD_ERR_DEVICE, "low-pass kernel could not be launched with " + std::to_string(p.max_taps) + " taps");    // (plan_call admits no such call)
        HDK(launch_symbols, qb, S, p.max_m, p.max_new, e->max_R, e->tail.p, e->tail_cap, e->d_symstate.p, e->flipmask.p, e->weight.p, e->d_sym.p,
                           r.dcall, sl.h_slots.dev, e->slot_words, e->flips_cap ? e->flips_dbg.p : nullptr, e->flips_cap, e->min_R, sl.seq, ev_ride ? sl.ev_done : nullptr,
                           e->demod_ck_acc.p);
    }
    if (sl.timed) HD_HIP(hipEventRecord(sl.t3, qb));
    if (r.spectrum_on_qc) HD_HIP(hipStreamWaitEvent(qb, sl.ev_spec, 0));      // the call is complete when its spectra are
    if (!ev_ride) HD_HIP(hipEventRecord(sl.ev_done, qb));
    HD_HIP(hipGetLastError());
    return HD_OK;
}

// The call is enqueued: the planned mirror becomes the streams', the slot goes in flight, the buffers turn.
void commit_call(hd_engine* e, hd_engine::CallSlot& sl, const CallPlan& p, const CallRoute& r)
{
    e->mirror.swap(e->mirror_next);
    const bool in_ring = demod_in_ring(e, r.route);
    const bool lazy = e->lazy_spectra && r.route != Route::separate;      // (the spectrum launches of the separate kernels store what they transform)
    for (uint32_t s = 0; s < e->S; ++s) {
        SizeState& sz = e->mirror[s];
        sz.demod_in_ring = in_ring;
        if (hd::sc_fft_run(sl.h_call.p[s])) sz.spec_stale = lazy;
    }
    sl.busy = true;
    if (r.route == Route::step) {   // this call's tails ride in the next call's launch
        e->pend.valid = true; e->pend.ta = r.ta_step; e->pend.slot = (int)(e->calls % hd_engine::kSlots);
        e->pend.r2 = (int)p.R2; e->pend.t2 = (int)p.T2; e->pend_max_taps = p.max_taps;
    }
    e->cur = (e->cur + 1) % 3;
    e->carry_cur ^= 1;
    if (p.max_in && p.nst) e->hist_cur ^= 1;
    ++e->calls;
}

// The sizes hd_process_device accepts: checked before anything is enqueued
int check_sizes(const hd_engine* e, const uint32_t* n_per_stream, uint32_t n_uniform)
{
    const size_t nst = e->stages.size();
    const uint32_t T1 = nst > 0 ? (uint32_t)e->stages[0].taps.size() : 0, T2 = nst > 1 ? (uint32_t)e->stages[1].taps.size() : 0;
    const uint32_t R1 = nst > 0 ? e->stages[0].ratio : 1;
    for (uint32_t s = 0; s < e->S; ++s) {
        const uint32_t n = n_per_stream ? n_per_stream[s] : n_uniform;
        if (n > e->cfg.max_chunk) return fail(HD_ERR_CAPACITY, "more samples than max_chunk");
        if (n % e->D) return fail(HD_ERR_INVALID, "sample count must be a multiple of the decimation factor (queue the remainder)");
        if (n && nst > 0 && n + 1 < T1) return fail(HD_ERR_UNSUPPORTED, "chunk shorter than the first stage's history (undefined in the reference)");
        if (n && nst > 1 && n / R1 + 1 < T2) return fail(HD_ERR_UNSUPPORTED, "chunk shorter than the second stage's history (undefined in the reference)");
    }
    return HD_OK;
}

}  // namespace

extern "C" {

int hd_flush(hd_engine* e)
{
    if (!e) return fail(HD_ERR_INVALID, "null engine");
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    if (e->in_callback) return fail(HD_ERR_INVALID, "hd_flush cannot be called from a sentence / character callback (the delivery it would join is the one running)");
    HD_HIP(hipSetDevice(e->cfg.device));
    const int rc = flush_locked(e);
    if (e->device_failed) return fail(HD_ERR_DEVICE, "this engine is in its failed state (" + e->fail_cause + ") -- destroy the engine");
    return rc;
}

int hd_process_device(hd_engine* e, const void* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n_uniform)
{
    if (!e) return fail(HD_ERR_INVALID, "null engine");
    if (!d_iq) return fail(HD_ERR_INVALID, "null IQ pointer");
    if ((reinterpret_cast<uintptr_t>(d_iq) & 15) || (stride & 1)) return fail(HD_ERR_INVALID, "IQ base must be 16-byte aligned and stream_stride even");
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    if (e->in_callback) return fail(HD_ERR_INVALID, "hd_process_* cannot be called from a sentence / character callback");   // (a nested delivery would count the slot being delivered twice)
    if (e->device_failed) return fail(HD_ERR_DEVICE, "this engine is in its failed state (" + e->fail_cause + "): no new calls are accepted -- destroy the engine");
    const auto h0 = std::chrono::steady_clock::now();
    HD_HIP(hipSetDevice(e->cfg.device));

    // ---- validate first: a call refused before anything is enqueued leaves every stream, e->calls and the buffer rotations as they were
    if (const int rc = check_sizes(e, n_per_stream, n_uniform)) return rc;
    // ---- every drain ahead of planning (collect() writes the mirror): a free slot -- cannot be wanting with depth <= 3, but never reuse a slot in
    // flight --, then the tables: control-plane changes (new low-pass design, new symbol parameters) rewrite device tables the previous call's back half
    // may still be reading.  Rare.
    if (const int rc = deliver(e, hd_engine::kSlots - 1)) return rc;
    bool tables_dirty = e->sym_dirty;
    for (uint32_t s = 0; s < e->S && !tables_dirty; ++s) tables_dirty = e->st[s].taps_dirty;
    if (tables_dirty) { if (const int rc = flush_locked(e)) return rc; }
    hd_engine::CallSlot& sl = e->slot[e->calls % hd_engine::kSlots];
    CallPlan p;
    bool redesigned = false;
    do {   // a low-pass redesign while planning (a stream's batch size changed): drain, and plan again -- the second pass finds the designs unchanged
        if (redesigned) { if (const int rc = flush_locked(e)) return rc; }
        if (const int rc = plan_call(e, sl, n_per_stream, n_uniform, p, redesigned)) return rc;
    } while (redesigned);
    CallRoute r;
    route_call(e, sl, p, r);

    // ---- enqueue.  From the first upload on, a failure leaves device-side histories part-advanced against the mirror: the engine goes into its failed state.
    const float2* iq = static_cast<const float2*>(d_iq);
    int rc = enqueue_uploads(e, sl, r);
    if (!rc) rc = r.route == Route::step ? enqueue_step(e, sl, p, r, iq, stride) : enqueue_front(e, sl, p, r, iq, stride);
    if (!rc && r.route != Route::step) rc = enqueue_back(e, sl, p, r);
    if (rc) {
        e->device_failed = true;
        e->fail_cause = "call " + std::to_string(e->calls) + " was enqueued in part (" + g_err + ")";
        return rc;
    }
    commit_call(e, sl, p, r);
    e->last_timing.host_enqueue_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h0).count();

    // ---- deliver.  Synchronous: this call.  Pipelined: keep up to two calls in flight and deliver the oldest one's results now (its host stage overlaps the
    // GPU work of the newer calls, and the GPU always has the next call queued).  Step launches run strictly in order on one queue, so how far the host
    // lags behind with the results is only a matter of the host-visible slots: pipeline = 2 keeps three calls undelivered instead of two -- results one
    // call later still, and a host that is held up for a whole launch (a descheduled thread, a burst of sentences) no longer leaves the queue empty.
    const uint64_t depth = !e->cfg.pipeline ? 0u : (r.route == Route::step && e->cfg.pipeline >= 2) ? 3u : 2u;
    return deliver(e, depth);
}

void* hd_pinned_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void hd_pinned_free(void* p) { if (p) (void)hipHostFree(p); }

int hd_process_host(hd_engine* e, const float* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n_uniform)
{
    if (!e) return fail(HD_ERR_INVALID, "null engine");
    if (!iq) return fail(HD_ERR_INVALID, "null IQ pointer");
    std::lock_guard<std::recursive_mutex> lock(e->mtx);   // (recursive: hd_process_device below takes it again)
    if (e->in_callback) return fail(HD_ERR_INVALID, "hd_process_* cannot be called from a sentence / character callback");
    HD_HIP(hipSetDevice(e->cfg.device));
    // Synchronous delivery from page-locked, mapped memory (hd_pinned_alloc, or any hipHostMalloc'ed / registered buffer): the kernels are done when the
    // call returns, so the first decimation stage may read the caller's buffer in place over PCIe -- no staging copy in front of it.  (Pageable memory,
    // batch mode -- the caller may reuse the buffer while the call is still queued -- or a base the 16-byte loads cannot take: the copy below.)
    if (!e->cfg.pipeline && !(reinterpret_cast<uintptr_t>(iq) & 15) && !(stride & 1)) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, iq) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) {
            ++e->host_calls_in_place;
            return hd_process_device(e, at.devicePointer, stride, n_per_stream, n_uniform);
        }
        (void)hipGetLastError();                          // (an ordinary pointer: the query's error is not the call's)
    }
    const size_t dstride = e->cfg.max_chunk;
    // validate the sizes before anything is queued (hd_process_device checks the rest and leaves every stream untouched when it refuses a call)
    for (uint32_t s = 0; s < e->S; ++s)
        if ((n_per_stream ? n_per_stream[s] : n_uniform) > e->cfg.max_chunk) return fail(HD_ERR_CAPACITY, "more samples than max_chunk");
    // The copy stream is created on first use, AFTER the engine's compute streams: HIP deals streams to a handful of hardware queues in
    // creation order, and a copy stream created in between put the two compute streams on one queue (their kernels took turns).
    if (!e->qh) HD_HIP(hipStreamCreateWithFlags(&e->qh, hipStreamNonBlocking));
    const int j = (int)(e->host_calls & 1u);
    if (j == 1 && !e->staging2.p) {
        HD_HIP(e->staging2.alloc((size_t)e->S * e->cfg.max_chunk));
        HD_HIP(hipDeviceSynchronize());      // the allocation's memset runs on the null stream: it must not trail the copy below
    }
    float2* dst = j ? e->staging2.p : e->staging.p;
    if (e->staging_used[j]) HD_HIP(hipStreamWaitEvent(e->qh, e->ev_staging_free[j], 0));    // the call that read this slab two calls ago is past its stage 1
    if (!stride) {
        // every stream reads the same recording: one copy, and the streams read it with stride 0 as well
        uint32_t n_max = n_uniform;
        if (n_per_stream) { n_max = 0; for (uint32_t s = 0; s < e->S; ++s) n_max = std::max(n_max, n_per_stream[s]); }
        if (n_max) HD_HIP(hipMemcpyAsync(dst, iq, (size_t)n_max * sizeof(float2), hipMemcpyHostToDevice, e->qh));
    } else if (!n_per_stream) {
        if (n_uniform)
            HD_HIP(hipMemcpy2DAsync(dst, dstride * sizeof(float2), iq, stride * sizeof(float2), (size_t)n_uniform * sizeof(float2),
                                    e->S, hipMemcpyHostToDevice, e->qh));
    } else {
        for (uint32_t s = 0; s < e->S; ++s) {
            const uint32_t n = n_per_stream[s];
            if (n) HD_HIP(hipMemcpyAsync(dst + (size_t)s * dstride, iq + 2 * (size_t)s * stride, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, e->qh));
        }
    }
    HD_HIP(hipEventRecord(e->ev_copy[j], e->qh));
    HD_HIP(hipStreamWaitEvent(e->qa, e->ev_copy[j], 0));
    HD_HIP(hipEventSynchronize(e->ev_copy[j]));          // from here on the caller's buffer is his again
    const int rc = hd_process_device(e, dst, stride ? dstride : 0, n_per_stream, n_uniform);
    HD_HIP(hipEventRecord(e->ev_staging_free[j], e->qa));
    e->staging_used[j] = true;
    ++e->host_calls;
    return rc;
}

}  // extern "C"

namespace {

// hd_process_host_fmt / hd_process_device_fmt of a packed format: the packed rows -- the caller's device buffer, the caller's page-locked mapped buffer
// (synchronous engine) or the packed slab a host buffer was copied into -- are unpacked on qh into the staging slab of this call's turn, and the
// call goes on as hd_process_host's does behind its copy: hd_process_device on the slab.
int process_packed(hd_engine* e, int fmt, const void* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n_uniform, bool device)
{
    if (!e) return fail(HD_ERR_INVALID, "null engine");
    const size_t bps = hd::iq_bytes(fmt);
    if (!bps || fmt == HD_IQ_CF32) return fail(HD_ERR_INVALID, "unknown IQ format (HD_IQ_CF32, HD_IQ_CS16, HD_IQ_CS8, HD_IQ_CU8)");
    if (!iq) return fail(HD_ERR_INVALID, "null IQ pointer");
    if (reinterpret_cast<uintptr_t>(iq) & (bps - 1)) return fail(HD_ERR_INVALID, "packed IQ base must be aligned to one sample (4 bytes cs16, 2 bytes cs8 / cu8)");
    std::lock_guard<std::recursive_mutex> lock(e->mtx);   // (recursive: hd_process_device below takes it again)
    if (e->in_callback) return fail(HD_ERR_INVALID, "hd_process_* cannot be called from a sentence / character callback");
    if (e->device_failed) return fail(HD_ERR_DEVICE, "this engine is in its failed state (" + e->fail_cause + "): no new calls are accepted -- destroy the engine");
    HD_HIP(hipSetDevice(e->cfg.device));
    // everything hd_process_device would refuse the sizes for is refused here, before anything is queued
    if (const int rc = check_sizes(e, n_per_stream, n_uniform)) return rc;
    const uint32_t S = e->S;
    const size_t dstride = e->cfg.max_chunk;
    uint32_t n_max = n_uniform;
    if (n_per_stream) { n_max = 0; for (uint32_t s = 0; s < S; ++s) n_max = std::max(n_max, n_per_stream[s]); }
    const int j = (int)(e->host_calls & 1u);
    if (j == 1 && !e->staging2.p) {
        HD_HIP(e->staging2.alloc((size_t)S * e->cfg.max_chunk));
        HD_HIP(hipDeviceSynchronize());      // the allocation's memset runs on the null stream: it must not trail the unpack below
    }
    if (!e->unpack_n.p) { HD_HIP(e->unpack_n.alloc(S)); HD_HIP(hipDeviceSynchronize()); }
    float2* dst = j ? e->staging2.p : e->staging.p;
    const void* src = iq;
    size_t sstride = stride;
    bool in_place = device;
    if (!device && !e->cfg.pipeline) {       // synchronous engine, page-locked mapped memory: the unpack reads the caller's buffer in place over PCIe
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, iq) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) {
            src = at.devicePointer;
            in_place = true;
            ++e->host_calls_in_place;
        } else {
            (void)hipGetLastError();         // (an ordinary pointer: the query's error is not the call's)
        }
    }
    // Synchronous engine with nothing to copy: its one queue is idle between calls and the call is done when it returns, so the unpack goes straight in
    // front of stage 1 on that queue -- no event between two queues (~18 us) and no host wait for it.  Everything else: the copy queue, as hd_process_host.
    const bool direct = in_place && !e->cfg.pipeline;
    if (!direct && !e->qh) HD_HIP(hipStreamCreateWithFlags(&e->qh, hipStreamNonBlocking));   // (created on first use: see hd_process_host)
    hipStream_t q = direct ? e->qa : e->qh;
    if (e->staging_used[j] && !direct) HD_HIP(hipStreamWaitEvent(q, e->ev_staging_free[j], 0));    // the call that read this slab two calls ago is past its stage 1
    if (!in_place) {
        // the packed bytes into the packed slab of this turn, in the three shapes of hd_process_host's copy
        const size_t need = (size_t)S * dstride * bps;
        if (e->packed_bytes[j] < need) {
            HD_HIP(hipStreamSynchronize(q));          // (a wider format than the slab was made for: nothing may still read the old one)
            if (e->packed[j]) { (void)hipFree(e->packed[j]); e->packed[j] = nullptr; e->packed_bytes[j] = 0; }
            HD_HIP(hipMalloc(reinterpret_cast<void**>(&e->packed[j]), need));
            e->packed_bytes[j] = need;
        }
        unsigned char* pk = e->packed[j];
        const unsigned char* h = static_cast<const unsigned char*>(iq);
        if (!stride) {
            if (n_max) HD_HIP(hipMemcpyAsync(pk, h, (size_t)n_max * bps, hipMemcpyHostToDevice, q));
        } else if (!n_per_stream) {
            if (n_uniform) HD_HIP(hipMemcpy2DAsync(pk, dstride * bps, h, stride * bps, (size_t)n_uniform * bps, S, hipMemcpyHostToDevice, q));
        } else {
            for (uint32_t s = 0; s < S; ++s) {
                const uint32_t n = n_per_stream[s];
                if (n) HD_HIP(hipMemcpyAsync(pk + (size_t)s * dstride * bps, h + (size_t)s * stride * bps, (size_t)n * bps, hipMemcpyHostToDevice, q));
            }
        }
        src = pk;
        sstride = stride ? dstride : 0;
    }
    if (!stride) {
        // one shared row: converted once, and the streams read it with stride 0
        if (!hd::launch_iq_unpack(q, fmt, 1, n_max, src, 0, nullptr, n_max, dst, 0)) return fail(HD_ERR_INVALID, "no unpack kernel for this IQ format");
    } else {
        const uint32_t* d_n = nullptr;
        if (n_per_stream) {
            HD_HIP(hipMemcpyAsync(e->unpack_n.p, n_per_stream, (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice, q));
            d_n = e->unpack_n.p;
        }
        if (!hd::launch_iq_unpack(q, fmt, S, n_max, src, sstride, d_n, n_uniform, dst, dstride)) return fail(HD_ERR_INVALID, "no unpack kernel for this IQ format");
    }
    HD_HIP(hipGetLastError());
    if (!direct) {
        HD_HIP(hipEventRecord(e->ev_copy[j], q));
        HD_HIP(hipStreamWaitEvent(e->qa, e->ev_copy[j], 0));
        HD_HIP(hipEventSynchronize(e->ev_copy[j]));      // from here on the caller's buffer (and n_per_stream) is theirs again
    }
    const int rc = hd_process_device(e, dst, stride ? dstride : 0, n_per_stream, n_uniform);
    if (direct && rc) (void)hipStreamSynchronize(q);     // (a call refused behind the unpack: the caller's buffer is theirs again only when the unpack has read it)
    HD_HIP(hipEventRecord(e->ev_staging_free[j], e->qa));
    e->staging_used[j] = true;
    ++e->host_calls;
    return rc;
}

}  // namespace

extern "C" {

int hd_process_host_fmt(hd_engine* e, int fmt, const void* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n_uniform)
{
    if (fmt == HD_IQ_CF32) return hd_process_host(e, static_cast<const float*>(iq), stride, n_per_stream, n_uniform);
    return process_packed(e, fmt, iq, stride, n_per_stream, n_uniform, false);
}

int hd_process_device_fmt(hd_engine* e, int fmt, const void* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n_uniform)
{
    if (fmt == HD_IQ_CF32) return hd_process_device(e, d_iq, stride, n_per_stream, n_uniform);
    return process_packed(e, fmt, d_iq, stride, n_per_stream, n_uniform, true);
}

// Measurement and test hook (tools/micro/iq_format_rate.py, tests/test_gpu_iq_formats.py; not part of the ABI): one unpack launch straight into a buffer
// of the caller's, between two HIP events on the host-copy queue -- row r reads d_n[r] (a device array; null: n_uniform) samples at
// d_src + r * src_stride * bps and writes them at d_dst + r * dst_stride.  With fmt = HD_IQ_CF32: a device-to-device copy of rows * n_uniform * 8 bytes.
int hd_debug_iq_unpack_timed(hd_engine* e, int fmt, const void* d_src, size_t src_stride, const uint32_t* d_n, uint32_t n_uniform, uint32_t max_n,
                             uint32_t rows, void* d_dst, size_t dst_stride, float* ms)
{
    if (!e || !d_src || !d_dst || !ms) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    HD_HIP(hipSetDevice(e->cfg.device));
    if (!e->qh) HD_HIP(hipStreamCreateWithFlags(&e->qh, hipStreamNonBlocking));
    hipEvent_t t0 = nullptr, t1 = nullptr;
    HD_HIP(hipEventCreate(&t0));
    HD_HIP(hipEventCreate(&t1));
    HD_HIP(hipEventRecord(t0, e->qh));
    bool ok = true;
    if (fmt == HD_IQ_CF32) HD_HIP(hipMemcpyAsync(d_dst, d_src, (size_t)rows * n_uniform * sizeof(float2), hipMemcpyDeviceToDevice, e->qh));
    else ok = hd::launch_iq_unpack(e->qh, fmt, rows, max_n, d_src, src_stride, d_n, n_uniform, static_cast<float2*>(d_dst), dst_stride);
    HD_HIP(hipEventRecord(t1, e->qh));
    HD_HIP(hipEventSynchronize(t1));
    HD_HIP(hipEventElapsedTime(ms, t0, t1));
    (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
    HD_HIP(hipGetLastError());
    return ok ? HD_OK : fail(HD_ERR_INVALID, "unknown IQ format");
}

/* ---------------------------------------------------------------- batched file ingest -------------------------- */

int hd_ingest_run(hd_engine* e, hd_host_iqfiles* src, uint64_t max_rounds, uint64_t* samples_done)
{
    if (samples_done) *samples_done = 0;
    if (!e || !src) return fail(HD_ERR_INVALID, "null engine or file batch");
    const uint32_t S = e->S;
    if (src->batch.streams() != S) return fail(HD_ERR_INVALID, "the file batch must hold one file per stream");
    if (src->batch.chunk() > e->cfg.max_chunk) return fail(HD_ERR_CAPACITY, "file batch chunk larger than max_chunk");
    HD_HIP(hipSetDevice(e->cfg.device));
    constexpr int kSlabs = 4;      // round r's slab is refilled for round r+4: by then call r is delivered even with two calls in flight
    const size_t stride = src->batch.chunk();
    const int fmt = src->batch.fmt();                  // a packed batch keeps its slabs packed: hd_process_host_fmt unpacks them on the GPU
    struct Slab { void* iq = nullptr; std::vector<uint32_t> n; uint32_t alive = 0; };
    Slab slab[kSlabs];
    auto release = [&] { for (auto& b : slab) if (b.iq) (void)hipHostFree(b.iq); };
    for (auto& b : slab) {
        if (hipHostMalloc(&b.iq, (size_t)S * stride * src->batch.bytes_per_sample(), hipHostMallocDefault) != hipSuccess) {
            release();
            return fail(HD_ERR_DEVICE, "pinned slab allocation failed");
        }
        b.n.assign(S, 0);
    }
    std::mutex m;
    std::condition_variable cv;
    uint64_t filled = 0, consumed = 0;       // rounds read by the reader / handed back by the pump
    bool stop = false;
    src->batch.set_min_take(hd_min_chunk(e->D));      // a file tail shorter than the stage histories waits for the next round
    const bool looping = src->batch.looping();
    std::thread reader([&] {
        for (uint64_t r = 0; r < max_rounds; ++r) {       // never read past the stop: a later hd_ingest_run resumes where this one ended
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return stop || r < consumed + (uint64_t)kSlabs - 2; });   // two slabs may still belong to calls in flight
                if (stop) return;
            }
            Slab& b = slab[r % kSlabs];
            b.alive = src->batch.next_raw(b.iq, stride, b.n.data());
            {
                std::lock_guard<std::mutex> l(m);
                filled = r + 1;
            }
            cv.notify_all();
            if (!b.alive && !looping) return;
        }
    });
    int rc = HD_OK;
    uint64_t total = 0;
    for (uint64_t r = 0; r < max_rounds; ++r) {
        {
            std::unique_lock<std::mutex> l(m);
            cv.wait(l, [&] { return filled > r; });
        }
        Slab& b = slab[r % kSlabs];
        if (!b.alive) {
            if (!looping) break;
            // looping files of equal length a whole number of chunks long: the reference's one empty read before the rewind
            { std::lock_guard<std::mutex> l(m); consumed = r + 1; }
            cv.notify_all();
            continue;
        }
        bool uniform = true;
        for (uint32_t s = 1; s < S; ++s) uniform = uniform && b.n[s] == b.n[0];
        rc = hd_process_host_fmt(e, fmt, b.iq, stride, uniform ? nullptr : b.n.data(), uniform ? b.n[0] : 0);
        if (rc) break;
        for (uint32_t s = 0; s < S; ++s) total += b.n[s];
        {
            std::lock_guard<std::mutex> l(m);
            consumed = r + 1;
        }
        cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> l(m);
        stop = true;
    }
    cv.notify_all();
    reader.join();
    const int rf = hd_flush(e);      // nothing may still copy from the slabs when they are freed
    HD_HIP(hipDeviceSynchronize());
    release();
    if (samples_done) *samples_done = total;
    return rc ? rc : rf;
}

/* ---------------------------------------------------------------- results -------------------------------------- */

static size_t copy_out(const std::string& s, char* buf, size_t cap)
{
    if (buf && cap) { const size_t n = std::min(cap - 1, s.size()); std::memcpy(buf, s.data(), n); buf[n] = 0; }
    return s.size();
}
static size_t take_out(std::string& s, char* buf, size_t cap)
{
    const size_t n = copy_out(s, buf, cap);
    if (buf && cap > n) s.clear();
    return n;
}

size_t hd_stream_rtty(hd_engine* e, uint32_t s, char* buf, size_t cap)
{ if (check_stream(e, s)) return 0; std::lock_guard<std::recursive_mutex> l(e->mtx); return copy_out(e->st[s].text.stream, buf, cap); }
size_t hd_stream_last_sentence(hd_engine* e, uint32_t s, char* buf, size_t cap)
{ if (check_stream(e, s)) return 0; std::lock_guard<std::recursive_mutex> l(e->mtx); return copy_out(e->st[s].text.last_sentence, buf, cap); }
size_t hd_stream_take_sentences(hd_engine* e, uint32_t s, char* buf, size_t cap)
{ if (check_stream(e, s)) return 0; std::lock_guard<std::recursive_mutex> l(e->mtx); return take_out(e->st[s].text.ok_log, buf, cap); }
size_t hd_stream_take_matches(hd_engine* e, uint32_t s, char* buf, size_t cap)
{ if (check_stream(e, s)) return 0; std::lock_guard<std::recursive_mutex> l(e->mtx); return take_out(e->st[s].text.match_log, buf, cap); }
size_t hd_stream_take_chars(hd_engine* e, uint32_t s, char* buf, size_t cap)
{ if (check_stream(e, s)) return 0; std::lock_guard<std::recursive_mutex> l(e->mtx); return take_out(e->st[s].text.char_log, buf, cap); }

int hd_stream_afc(hd_engine* e, uint32_t s, hd_afc_info* out)
{
    if (int r = check_stream(e, s)) return r;
    if (!out) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    const StreamHost& st = e->st[s];
    out->frequency_correction = st.afc.correction; out->shift_hz = st.afc.shift_hz;
    out->noise_floor = st.afc.noise_floor; out->noise_variance = st.afc.noise_sigma;
    out->peak_left = st.afc.gui_left; out->peak_right = st.afc.gui_right; out->spectra = st.spectra;
    return HD_OK;
}

// Batch mode (hd_engine::lazy_spectra): the spectra the stream tails transformed but did not store -- one spectrum launch over the streams whose stored
// spectrum is older than their last completed collection buffer, which is still as that tail read it.  Same transform body, same inputs: the bytes a
// tail would have stored.  The statistics were delivered with the call (null pointer: not written again).  The pipeline is drained when this runs.
static int refresh_spectra(hd_engine* e)
{
    if (!e->lazy_spectra) return HD_OK;
    bool any = false;
    for (uint32_t s = 0; s < e->S; ++s) {
        const SizeState& sz = e->mirror[s];
        e->h_spec_call.p[s].fft_run = sz.spec_stale ? hd::sc_pack_fft_run(1, sz.spec_buf) : 0u;
        any |= sz.spec_stale;
    }
    if (!any) return HD_OK;
    HD_HIP(hipSetDevice(e->cfg.device));
    hd::launch_spectrum_wave(e->qa, e->S, e->fft_in.p, e->fft_tw.p, e->spec.p, e->power.p, nullptr, e->h_spec_call.dev, e->fsd, e->bins_sep, 0u);
    HD_HIP(hipGetLastError());
    HD_HIP(hipStreamSynchronize(e->qa));
    for (SizeState& sz : e->mirror) sz.spec_stale = false;
    return HD_OK;
}
// A data getter in two steps: refuse it inside a callback and drain the pipeline (getter_ready), then copy (copy_to_host).  fetch is both.
static bool getter_ready(hd_engine* e)
{
    if (e->in_callback) { fail(HD_ERR_INVALID, "data getters cannot be called from a sentence / character callback (text getters can)"); return false; }
    (void)flush_locked(e);                                  // pipelined mode: wait for the call in flight
    return true;
}
static bool copy_to_host(hd_engine* e, void* host, const void* dev, size_t bytes)
{
    return !bytes || (hipSetDevice(e->cfg.device) == hipSuccess && hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess);
}
static size_t fetch(hd_engine* e, const void* dev, size_t count, size_t elem, void* host, size_t cap)
{
    if (!getter_ready(e)) return 0;
    const size_t n = std::min(count, cap);
    if (!n || !host) return count;
    return copy_to_host(e, host, dev, n * elem) ? count : 0;
}

static size_t fetch_spectrum(hd_engine* e, const void* dev, size_t elem, void* host, size_t cap)
{
    if (!getter_ready(e) || refresh_spectra(e) != HD_OK) return 0;
    const size_t n = std::min<size_t>(hd::kFftBins, cap);
    if (!n || !host) return hd::kFftBins;
    return copy_to_host(e, host, dev, n * elem) ? (size_t)hd::kFftBins : 0;
}

size_t hd_stream_spectrum(hd_engine* e, uint32_t s, float* iq, size_t cap)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    if (!e->cfg.enable_spectrum || !e->st[s].have_spectrum) return 0;
    return fetch_spectrum(e, e->spec.p + (size_t)s * hd::kFftBins, sizeof(float2), iq, cap);
}
size_t hd_stream_power(hd_engine* e, uint32_t s, float* p, size_t cap)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    if (!e->cfg.enable_spectrum || !e->st[s].have_spectrum) return 0;
    return fetch_spectrum(e, e->power.p + (size_t)s * hd::kFftBins, sizeof(float), p, cap);
}
size_t hd_stream_demodulated(hd_engine* e, uint32_t s, float* v, size_t cap)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    const SizeState& sz = e->mirror[s];
    if (!sz.demod_in_ring) return fetch(e, e->demod.p + (size_t)s * (e->demod.n / e->S), sz.last_m, sizeof(float), v, cap);
    // A stream tail of a batch-mode engine left the call's output in the symbol ring only (fill_tail): the last_m samples in front of the ring's append
    // position, which is base + held of the stream's SymState once the pipeline is drained (the tail's symbol search moves base and held, never their sum).
    if (!getter_ready(e)) return 0;
    const size_t count = sz.last_m, n = std::min(count, cap);
    if (!n || !v) return count;
    hd::SymState st;
    if (!copy_to_host(e, &st, e->d_symstate.p + s, sizeof(st))) return 0;
    const float* ring = e->tail.p + (size_t)s * e->tail_cap;
    const uint32_t first = (st.base + st.held - (uint32_t)count) & (e->tail_cap - 1u);       // (count <= m_cap < tail_cap)
    const size_t n0 = std::min<size_t>(n, e->tail_cap - first);                              // up to the ring's end, then from its start
    return copy_to_host(e, v, ring + first, n0 * sizeof(float)) && copy_to_host(e, v + n0, ring, (n - n0) * sizeof(float)) ? count : 0;
}
size_t hd_stream_decimated(hd_engine* e, uint32_t s, float* iq, size_t cap)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    const SizeState& sz = e->mirror[s];
    const float2* src = e->fbuf[sz.last_buf].p + (size_t)s * e->fbuf_stride + e->fir_hist_cap + sz.last_pend_before;
    return fetch(e, src, sz.last_n2, sizeof(float2), iq, cap);
}
size_t hd_stream_filtered(hd_engine* e, uint32_t s, float* iq, size_t cap)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    if (!e->cfg.keep_filtered) return 0;
    return fetch(e, e->filtered.p + (size_t)s * (e->demod.n / e->S), e->mirror[s].last_m, sizeof(float2), iq, cap);
}
size_t hd_stream_bits(hd_engine* e, uint32_t s, uint8_t* bits, size_t cap)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    const StreamHost& st = e->st[s];
    for (uint32_t i = 0; i < st.last_nbits && i < cap; ++i) bits[i] = (st.last_words[i >> 5] >> (i & 31)) & 1u;
    return st.last_nbits;
}
size_t hd_stream_flips(hd_engine* e, uint32_t s, uint32_t* flips, size_t cap)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    if (!e->flips_cap) return 0;
    const size_t n = std::min<size_t>(e->st[s].last_nflips, e->flips_cap);
    return fetch(e, e->flips_dbg.p + (size_t)s * e->flips_cap, n, sizeof(uint32_t), flips, cap);
}
size_t hd_stream_fir_taps(hd_engine* e, uint32_t s, float* taps, size_t cap)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    const auto& t = e->st[s].lp.taps;
    if (taps) std::memcpy(taps, t.data(), std::min(cap, t.size()) * sizeof(float));
    return t.size();
}
uint64_t hd_stream_bits_total(hd_engine* e, uint32_t s)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    return e->st[s].bits_total;
}
uint64_t hd_stream_flip_list_full(hd_engine* e, uint32_t s)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    return e->st[s].flip_list_full;
}
int hd_stream_demod_checksum(hd_engine* e, uint32_t s, uint64_t* call_index, uint32_t* n, uint32_t ck[2])
{
    if (check_stream(e, s)) return HD_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    const StreamHost& st = e->st[s];
    if (call_index) *call_index = st.demod_ck_call;
    if (n) *n = st.demod_ck_n;
    if (ck) { ck[0] = st.demod_ck[0]; ck[1] = st.demod_ck[1]; }
    return HD_OK;
}
int hd_stream_demod_checksum_total(hd_engine* e, uint32_t s, uint64_t* calls, uint64_t* calls_without, uint64_t* hash)
{
    if (check_stream(e, s)) return HD_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    const StreamHost& st = e->st[s];
    if (calls) *calls = st.demod_ck_calls;
    if (calls_without) *calls_without = st.demod_ck_unknown;
    if (hash) *hash = st.demod_ck_hash;
    return HD_OK;
}
uint32_t hd_stream_symbol_backlog(hd_engine* e, uint32_t s)
{
    if (check_stream(e, s)) return 0;
    std::lock_guard<std::recursive_mutex> l(e->mtx);
    return e->st[s].held;
}

}  // extern "C"

