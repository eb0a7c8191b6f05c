// The objects that read a wideband capture beside the decode pipeline: the survey (kernels/survey.hip, host/survey.hpp) and the waterfall
// (kernels/waterfall.hip, host/waterfall.hpp).  Both run the survey's kernel over 4096-sample segments on a queue of their own and take IQ through
// the same doors -- cf32 or packed, from device or host memory -- so they share one feed: WideFeed and feed_push.
#include <cstdlib>

#include "engine_state.h"
#include "host/iq_convert.hpp"
#include "host/survey.hpp"
#include "host/waterfall.hpp"
#include "kernels/survey.h"
#include "kernels/waterfall.h"

using hd::eng::enter;
using hd::eng::is_device_pointer;

namespace {

// What a wideband object feeds its launches from.
struct WideFeed {
    hd_engine* e = nullptr;
    hipStream_t q = nullptr;               // the object's own queue: launches, staging copies and the read-backs
    const float2* tw = nullptr;            // the engine's twiddles, or own_tw where the engine computes no spectra
    DevBuf<float2> own_tw;
    DevBuf<float> win;                     // [4096] the window table
    DevBuf<float2> slab;                   // host and packed pushes: staging for kSlabSegs segments, allocated by the first push that needs it
    DevBuf<unsigned char> pslab;           // packed HOST pushes: the same segments packed (sized for cs16), allocated by the first of them
    static constexpr uint32_t kSlabSegs = 256;   // whole segments one staging copy carries ((256 + 1) hops = 4 MiB + 16 KiB)

    // The queue and the two tables.  w, tw_host: the tables on the host, the creator's locals -- their uploads are enqueued, not waited for: the
    // creator adds its own and waits for q once.  (Plain allocations, filled on q: nothing here runs on the null stream or waits for the engine's queues.)
    int create(hd_engine* engine, std::vector<float>& w, std::vector<float2>& tw_host)
    {
        e = engine;
        HD_HIP(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
        w.resize(hd::kSurveyBins);
        hd::survey_window(w.data());
        HD_HIP(win.alloc_unfilled(w.size()));
        if (const int rc = hd::eng::engine_or_own_twiddles(e, own_tw, tw_host, q, &tw)) return rc;
        HD_HIP(hipMemcpyAsync(win.p, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, q));
        return HD_OK;
    }
    ~WideFeed() { if (q) (void)hipStreamDestroy(q); }     // (the object's destroy has waited for q: the buffers, destroyed behind this, are idle)
};

// The argument checks of a push, in the order process_packed (engine.cpp) uses: format, null, alignment -- then the caller takes the lock.
int check_push_args(int fmt, const void* iq, bool device)
{
    const size_t bps = hd::iq_bytes(fmt);
    if (!bps) return fail(HD_ERR_INVALID, "unknown IQ format (HD_IQ_CF32, HD_IQ_CS16, HD_IQ_CS8, HD_IQ_CU8)");
    if (!iq) return fail(HD_ERR_INVALID, "null IQ pointer");
    if (fmt == HD_IQ_CF32) {
        if (device && (reinterpret_cast<uintptr_t>(iq) & 7)) return fail(HD_ERR_INVALID, "IQ base must be 8-byte aligned");
    } else if (reinterpret_cast<uintptr_t>(iq) & (bps - 1))
        return fail(HD_ERR_INVALID, "packed IQ base must be aligned to one sample (4 bytes cs16, 2 bytes cs8 / cu8)");
    return HD_OK;
}

// The n_seg >= 1 segments of one push reach enqueue(x, base_seg, seg0, seg1): segments [seg0, seg1) of the push, read from x, where x[0] is sample
// 2048 base_seg of the push and seg0 - base_seg is a multiple of `unit`.  Device cf32 is one piece, read in place.  Everything else goes through the
// slab in pieces of (kSlabSegs / unit) * unit segments: whole runs (survey) or rows (waterfall) of `unit` segments, so every wave sums the segments
// it would have summed in one device push, in the same order.  Copies, unpacks and launches share q: the slab is overwritten only behind the launch
// that read it.  Nothing here waits for q.
template <typename Enqueue>
int feed_push(WideFeed& f, int fmt, const void* iq, bool device, uint64_t n_seg, uint32_t unit, Enqueue enqueue)
{
    if (device && !is_device_pointer(iq)) return fail(HD_ERR_INVALID, "IQ pointer is not device memory (the _host calls take host memory)");
    const bool packed = fmt != HD_IQ_CF32;
    if (device && !packed) return enqueue(static_cast<const float2*>(iq), 0, 0, n_seg);
    const size_t bps = hd::iq_bytes(fmt);
    const size_t slab_samples = (size_t)(WideFeed::kSlabSegs + 1) * hd::kSurveyHop;
    if (!f.slab.p) HD_HIP(f.slab.alloc_unfilled(slab_samples));
    if (packed && !device && !f.pslab.p) HD_HIP(f.pslab.alloc_unfilled(slab_samples * 4u));
    const uint64_t per_slab = (uint64_t)(WideFeed::kSlabSegs / unit) * unit;      // at least one unit: unit <= 64 segments
    const unsigned char* p = static_cast<const unsigned char*>(iq);
    for (uint64_t s = 0; s < n_seg; s += per_slab) {
        const uint64_t s1 = std::min(n_seg, s + per_slab);
        const size_t samples = (size_t)(s1 - s + 1) * hd::kSurveyHop;
        const unsigned char* from = p + (size_t)s * hd::kSurveyHop * bps;
        if (!packed) {
            HD_HIP(hipMemcpyAsync(f.slab.p, from, samples * sizeof(float2), hipMemcpyHostToDevice, f.q));
        } else {
            if (!device) {
                HD_HIP(hipMemcpyAsync(f.pslab.p, from, samples * bps, hipMemcpyHostToDevice, f.q));
                from = f.pslab.p;
            }
            if (!hd::launch_iq_unpack(f.q, fmt, 1, (uint32_t)samples, from, 0, nullptr, (uint32_t)samples, f.slab.p, 0)) return fail(HD_ERR_INVALID, "no unpack kernel for this IQ format");
        }
        if (const int rc = enqueue(f.slab.p, s, s, s1)) return rc;
    }
    return HD_OK;
}

// hd_survey_destroy / hd_waterfall_destroy: the object's queue is waited for before anything is freed.
template <typename Obj>
void destroy(Obj* o)
{
    if (!o) return;
    hd_engine* e = o->feed.e;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    (void)hipSetDevice(e->cfg.device);
    if (o->feed.q) (void)hipStreamSynchronize(o->feed.q);
    delete o;
}

}  // namespace

/* ---------------------------------------------------------------- wideband survey (kernels/survey.hip) -------------------------- */

struct hd_survey {
    WideFeed feed;
    uint32_t runs_per_launch = 1024;       // HD_SURVEY_RUNS, read at creation
    DevBuf<float> partial;                 // [runs_per_launch][4096] float rows of the launch in flight (launches of one queue run in order)
    DevBuf<double> acc;                    // [4096], for the life of the survey
    double* h_acc = nullptr;               // page-locked landing place of the read-back
    double sum_w2 = 0;                     // sum of w^2, in double over the float table
    uint64_t segments = 0;
    ~hd_survey() { if (h_acc) (void)hipHostFree(h_acc); }
};

namespace {

// Segments [seg0, seg1) of a push whose run length is r, read from x (feed_push): launches of at most runs_per_launch runs, each followed by its reduction.
int survey_enqueue(hd_survey* sv, const float2* x, uint64_t base_seg, uint64_t seg0, uint64_t seg1, uint32_t r)
{
    for (uint64_t s = seg0; s < seg1;) {
        const uint64_t runs_left = (seg1 - s + r - 1) / r;
        const uint32_t runs = (uint32_t)std::min<uint64_t>(runs_left, sv->runs_per_launch);
        hd::launch_survey(sv->feed.q, runs, x, sv->feed.win.p, sv->feed.tw, sv->partial.p, s - base_seg, seg1 - base_seg, r);
        hd::launch_survey_reduce(sv->feed.q, sv->partial.p, runs, sv->acc.p);
        HD_HIP(hipGetLastError());
        s += (uint64_t)runs * r;
    }
    return HD_OK;
}

int survey_push(hd_survey* sv, int fmt, const void* iq, uint64_t n, bool device)
{
    if (!sv) return fail(HD_ERR_INVALID, "null survey");
    if (const int rc = check_push_args(fmt, iq, device)) return rc;
    std::lock_guard<std::recursive_mutex> lock(sv->feed.e->mtx);
    if (const int rc = enter(sv->feed.e)) return rc;
    const uint64_t n_seg = hd::survey_segments(n);
    if (!n_seg) return HD_OK;              // a push below one segment: before the device-pointer check
    const uint32_t r = hd::survey_run_len(n_seg, sv->runs_per_launch);     // the run length is the WHOLE push's, whatever the slabs cut it into
    if (const int rc = feed_push(sv->feed, fmt, iq, device, n_seg, r,
                                 [&](const float2* x, uint64_t base_seg, uint64_t seg0, uint64_t seg1) { return survey_enqueue(sv, x, base_seg, seg0, seg1, r); }))
        return rc;
    // The survey waits for its queue once, at the end of a push through the slab: from here on the caller's buffer is theirs again.  (A device cf32
    // push is not waited for.)
    if (!device || fmt != HD_IQ_CF32) HD_HIP(hipStreamSynchronize(sv->feed.q));
    sv->segments += n_seg;
    return HD_OK;
}

}  // namespace

extern "C" {

int hd_survey_create(hd_engine* e, hd_survey** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_survey> sv(new hd_survey);
    if (const int rc = enter(e)) return rc;
    if (const char* v = getenv("HD_SURVEY_RUNS")) sv->runs_per_launch = (uint32_t)std::min(std::max(atol(v), 1L), 4096L);
    std::vector<float> w;
    std::vector<float2> tw;
    if (const int rc = sv->feed.create(e, w, tw)) return rc;
    for (float v : w) sv->sum_w2 += (double)v * (double)v;
    HD_HIP(sv->partial.alloc_unfilled((size_t)sv->runs_per_launch * hd::kSurveyBins));
    HD_HIP(sv->acc.alloc_unfilled(hd::kSurveyBins));
    HD_HIP(hipHostMalloc(reinterpret_cast<void**>(&sv->h_acc), hd::kSurveyBins * sizeof(double), hipHostMallocDefault));
    HD_HIP(hipMemsetAsync(sv->acc.p, 0, hd::kSurveyBins * sizeof(double), sv->feed.q));
    HD_HIP(hipStreamSynchronize(sv->feed.q));   // (the tables above are locals)
    *out = sv.release();
    return HD_OK;
}

void hd_survey_destroy(hd_survey* sv) { destroy(sv); }

int hd_survey_reset(hd_survey* sv)
{
    if (!sv) return fail(HD_ERR_INVALID, "null survey");
    std::lock_guard<std::recursive_mutex> lock(sv->feed.e->mtx);
    if (const int rc = enter(sv->feed.e)) return rc;
    HD_HIP(hipMemsetAsync(sv->acc.p, 0, hd::kSurveyBins * sizeof(double), sv->feed.q));
    HD_HIP(hipStreamSynchronize(sv->feed.q));   // (what was pushed before is done with its buffers)
    sv->segments = 0;
    return HD_OK;
}

int hd_survey_push_device(hd_survey* sv, const void* d_iq, uint64_t n) { return survey_push(sv, HD_IQ_CF32, d_iq, n, true); }
int hd_survey_push_host(hd_survey* sv, const float* iq, uint64_t n) { return survey_push(sv, HD_IQ_CF32, iq, n, false); }
int hd_survey_push_device_fmt(hd_survey* sv, int fmt, const void* d_iq, uint64_t n) { return survey_push(sv, fmt, d_iq, n, true); }
int hd_survey_push_host_fmt(hd_survey* sv, int fmt, const void* iq, uint64_t n) { return survey_push(sv, fmt, iq, n, false); }

int hd_survey_power(hd_survey* sv, double* p, size_t cap, uint64_t* segments)
{
    if (!sv) return fail(HD_ERR_INVALID, "null survey");
    if (!p) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(sv->feed.e->mtx);
    if (const int rc = enter(sv->feed.e)) return rc;
    if (segments) *segments = sv->segments;
    if (cap < hd::kSurveyBins) return 0;
    HD_HIP(hipMemcpyAsync(sv->h_acc, sv->acc.p, hd::kSurveyBins * sizeof(double), hipMemcpyDeviceToHost, sv->feed.q));
    HD_HIP(hipStreamSynchronize(sv->feed.q));
    const double norm = (double)sv->segments * sv->sum_w2;
    for (uint32_t i = 0; i < hd::kSurveyBins; ++i) p[i] = sv->segments ? sv->h_acc[i] / norm : 0.0;
    return (int)hd::kSurveyBins;
}

// Measurement hook (tools/micro/survey_rate.py; not part of the ABI): hd_survey_push_device between two HIP events on the survey's queue.
int hd_debug_survey_push_timed(hd_survey* sv, const void* d_iq, uint64_t n, float* ms)
{
    if (!sv || !ms) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(sv->feed.e->mtx);
    if (const int rc = enter(sv->feed.e)) return rc;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    HD_HIP(hipEventCreate(&t0));
    HD_HIP(hipEventCreate(&t1));
    HD_HIP(hipEventRecord(t0, sv->feed.q));
    const int rc = hd_survey_push_device(sv, d_iq, n);
    HD_HIP(hipEventRecord(t1, sv->feed.q));
    HD_HIP(hipEventSynchronize(t1));
    HD_HIP(hipEventElapsedTime(ms, t0, t1));
    (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
    return rc;
}

void hd_survey_params_default(hd_survey_params* p) { if (p) hd::survey_params_default(p); }

int hd_survey_detect(hd_survey* sv, const hd_survey_params* p, hd_survey_candidate* out, uint32_t cap, uint32_t* found)
{
    if (found) *found = 0;
    if (!sv) return fail(HD_ERR_INVALID, "null survey");
    if (!p || !found || (cap && !out)) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(sv->feed.e->mtx);
    std::vector<double> pw(hd::kSurveyBins);
    uint64_t segs = 0;
    const int n = hd_survey_power(sv, pw.data(), pw.size(), &segs);
    if (n < 0) return n;
    const int rc = hd::survey_detect(pw.data(), segs, sv->feed.e->fs, p, out, cap, found);
    if (rc == HD_ERR_UNSUPPORTED) return fail(rc, "hd_survey_detect needs at least 16 segments and a floor above zero (" + std::to_string(segs) + " segments so far)");
    if (rc) return fail(rc, "hd_survey_detect: bad parameters or a NaN / negative power");
    return HD_OK;
}

}  // extern "C"

/* ---------------------------------------------------------------- waterfall (kernels/waterfall.hip, host/waterfall.hpp) ----------------- */

struct hd_waterfall {
    WideFeed feed;
    hd_waterfall_params par{};
    uint32_t guard_lo = 0, guard_hi = 0;   // the bins dc_guard_hz takes out
    DevBuf<float> factor;                  // [65] F[s]
    DevBuf<float> ring;                    // [rows_cap][4096]: row r lives at slot r % rows_cap
    DevBuf<uint32_t> hits;                 // [4096]
    DevBuf<hd::WaterfallRec> rec;          // [kChunkRows] the detector's records of the chunk in flight
    hd::WaterfallRec* h_rec = nullptr;     // their page-locked landing place
    DevBuf<uint32_t> d_seg;                // [kChunkRows] hd_waterfall_push_rows: the chunk's segment counts
    uint32_t* h_hits = nullptr;            // page-locked landing place of hd_waterfall_hits
    uint64_t samples = 0;                  // pushed since creation or reset
    uint64_t rows_counted = 0;             // unflagged rows
    std::vector<hd_waterfall_row> headers; // of all rows since creation or reset
    std::vector<uint32_t> marks;           // [rows][128]
    static constexpr uint32_t kChunkRows = 1024;  // most rows per launch and read-back (528 KiB of records): one k_survey wave per SIMD of the chip
    uint32_t chunk_rows = kChunkRows;             // HD_WATERFALL_CHUNK, read at creation: fewer, so that short pushes reach the several-launch shapes
    ~hd_waterfall()
    {
        if (h_rec) (void)hipHostFree(h_rec);
        if (h_hits) (void)hipHostFree(h_hits);
    }
};

namespace {

// The detector, the hit counters and the read-back for the n rows a launch has just put into the ring at `slot`; waits for the waterfall's queue and
// appends headers and marks.  d_seg: the rows' segment counts on the device (null: seg_full each, the last one seg_last); first[b], seg[b]: the same
// rows' first samples and segment counts for the headers.
int waterfall_detect_chunk(hd_waterfall* wf, uint32_t slot, uint32_t n, const uint32_t* d_seg, uint32_t seg_full, uint32_t seg_last, const uint64_t* first,
                           const uint32_t* seg)
{
    hipStream_t q = wf->feed.q;
    hd::launch_waterfall_detect(q, n, wf->ring.p + (size_t)slot * hd::kWaterfallBins, d_seg, seg_full, seg_last, wf->guard_lo, wf->guard_hi, wf->factor.p, wf->rec.p);
    hd::launch_waterfall_hits(q, wf->rec.p, n, wf->hits.p);
    HD_HIP(hipGetLastError());
    HD_HIP(hipMemcpyAsync(wf->h_rec, wf->rec.p, (size_t)n * sizeof(hd::WaterfallRec), hipMemcpyDeviceToHost, q));
    HD_HIP(hipStreamSynchronize(q));
    for (uint32_t b = 0; b < n; ++b) {
        const hd::WaterfallRec& r = wf->h_rec[b];
        hd_waterfall_row h{};
        h.first_sample = first[b]; h.segments = seg[b]; h.flags = r.flags; h.floor = r.floor; h.level = r.level; h.n_marked = r.n_marked;
        wf->headers.push_back(h);
        wf->marks.insert(wf->marks.end(), r.marks, r.marks + hd::kWaterfallWords);
        if (!r.flags) ++wf->rows_counted;
    }
    return HD_OK;
}

// Rows of segments [seg0, seg1) of a push, read from x (feed_push, unit = L): launches of the survey's kernel with run_len = L straight into the ring,
// cut where the ring wraps and at chunk_rows, each followed by its detector -- which waits for the queue, so a slab is free when this returns.
int waterfall_enqueue(hd_waterfall* wf, const float2* x, uint64_t base_seg, uint64_t seg0, uint64_t seg1)
{
    const uint32_t L = wf->par.slot_segments;
    uint64_t first[hd_waterfall::kChunkRows];
    uint32_t seg[hd_waterfall::kChunkRows];
    for (uint64_t s = seg0; s < seg1;) {
        const uint64_t rows_left = (seg1 - s + L - 1) / L;
        const uint32_t slot = (uint32_t)(wf->headers.size() % wf->par.rows_cap);
        const uint32_t n = (uint32_t)std::min<uint64_t>(rows_left, std::min<uint32_t>(wf->chunk_rows, wf->par.rows_cap - slot));
        hd::launch_survey(wf->feed.q, n, x, wf->feed.win.p, wf->feed.tw, wf->ring.p + (size_t)slot * hd::kWaterfallBins, s - base_seg, seg1 - base_seg, L);
        const uint64_t s_end = std::min<uint64_t>(seg1, s + (uint64_t)n * L);
        const uint32_t seg_last = (uint32_t)(s_end - (s + (uint64_t)(n - 1) * L));
        for (uint32_t b = 0; b < n; ++b) { first[b] = wf->samples + (s + (uint64_t)b * L) * hd::kSurveyHop; seg[b] = b + 1 == n ? seg_last : L; }
        if (const int rc = waterfall_detect_chunk(wf, slot, n, nullptr, L, seg_last, first, seg)) return rc;
        s = s_end;
    }
    return HD_OK;
}

int waterfall_push(hd_waterfall* wf, int fmt, const void* iq, uint64_t n, bool device)
{
    if (!wf) return fail(HD_ERR_INVALID, "null waterfall");
    if (const int rc = check_push_args(fmt, iq, device)) return rc;
    std::lock_guard<std::recursive_mutex> lock(wf->feed.e->mtx);
    if (const int rc = enter(wf->feed.e)) return rc;
    if (const uint64_t n_seg = hd::survey_segments(n))
        if (const int rc = feed_push(wf->feed, fmt, iq, device, n_seg, wf->par.slot_segments,
                                     [&](const float2* x, uint64_t base_seg, uint64_t seg0, uint64_t seg1) { return waterfall_enqueue(wf, x, base_seg, seg0, seg1); }))
            return rc;
    wf->samples += n;                      // (a push below one segment makes no row; its samples still count)
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_waterfall_params_default(hd_waterfall_params* p) { if (p) hd::waterfall_params_default(p); }
void hd_waterfall_track_params_default(hd_waterfall_track_params* p) { if (p) hd::waterfall_track_params_default(p); }

int hd_waterfall_create(hd_engine* e, const hd_waterfall_params* p, hd_waterfall** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_waterfall> wf(new hd_waterfall);
    if (p) wf->par = *p; else hd::waterfall_params_default(&wf->par);
    if (!hd::waterfall_params_ok(&wf->par)) return fail(HD_ERR_INVALID, "hd_waterfall_params: slot_segments 16..64, rows_cap >= 1, threshold_db and dc_guard_hz >= 0");
    if (!hd::waterfall_guard_range(e->fs, wf->par.dc_guard_hz, &wf->guard_lo, &wf->guard_hi)) return fail(HD_ERR_INVALID, "dc_guard_hz leaves no bin");
    if (const int rc = enter(e)) return rc;
    if (const char* v = getenv("HD_WATERFALL_CHUNK")) wf->chunk_rows = (uint32_t)std::min(std::max(atol(v), 1L), (long)hd_waterfall::kChunkRows);
    std::vector<float> w, f(hd::kWaterfallMaxSeg + 1, 0.0f);
    std::vector<float2> tw;
    if (const int rc = wf->feed.create(e, w, tw)) return rc;
    for (uint32_t s = 1; s <= hd::kWaterfallMaxSeg; ++s) f[s] = hd::waterfall_factor(wf->par.threshold_db, s);
    hipStream_t q = wf->feed.q;
    HD_HIP(wf->factor.alloc_unfilled(f.size()));
    HD_HIP(wf->ring.alloc_unfilled((size_t)wf->par.rows_cap * hd::kWaterfallBins));
    HD_HIP(wf->hits.alloc_unfilled(hd::kWaterfallBins));
    HD_HIP(wf->rec.alloc_unfilled(hd_waterfall::kChunkRows));
    HD_HIP(wf->d_seg.alloc_unfilled(hd_waterfall::kChunkRows));
    HD_HIP(hipHostMalloc(reinterpret_cast<void**>(&wf->h_rec), hd_waterfall::kChunkRows * sizeof(hd::WaterfallRec), hipHostMallocDefault));
    HD_HIP(hipHostMalloc(reinterpret_cast<void**>(&wf->h_hits), hd::kWaterfallBins * sizeof(uint32_t), hipHostMallocDefault));
    HD_HIP(hipMemcpyAsync(wf->factor.p, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice, q));
    HD_HIP(hipMemsetAsync(wf->hits.p, 0, hd::kWaterfallBins * sizeof(uint32_t), q));
    HD_HIP(hipStreamSynchronize(q));   // (the tables above are locals)
    *out = wf.release();
    return HD_OK;
}

void hd_waterfall_destroy(hd_waterfall* wf) { destroy(wf); }

int hd_waterfall_reset(hd_waterfall* wf)
{
    if (!wf) return fail(HD_ERR_INVALID, "null waterfall");
    std::lock_guard<std::recursive_mutex> lock(wf->feed.e->mtx);
    if (const int rc = enter(wf->feed.e)) return rc;
    HD_HIP(hipMemsetAsync(wf->hits.p, 0, hd::kWaterfallBins * sizeof(uint32_t), wf->feed.q));
    HD_HIP(hipStreamSynchronize(wf->feed.q));
    wf->headers.clear();
    wf->marks.clear();
    wf->samples = 0;
    wf->rows_counted = 0;
    return HD_OK;
}

int hd_waterfall_push_device(hd_waterfall* wf, const void* d_iq, uint64_t n) { return waterfall_push(wf, HD_IQ_CF32, d_iq, n, true); }
int hd_waterfall_push_host(hd_waterfall* wf, const float* iq, uint64_t n) { return waterfall_push(wf, HD_IQ_CF32, iq, n, false); }
int hd_waterfall_push_device_fmt(hd_waterfall* wf, int fmt, const void* d_iq, uint64_t n) { return waterfall_push(wf, fmt, d_iq, n, true); }
int hd_waterfall_push_host_fmt(hd_waterfall* wf, int fmt, const void* iq, uint64_t n) { return waterfall_push(wf, fmt, iq, n, false); }

int hd_waterfall_push_rows(hd_waterfall* wf, const float* rows, const uint32_t* segments, uint32_t n_rows, int device)
{
    if (!wf) return fail(HD_ERR_INVALID, "null waterfall");
    if (!rows || !segments) return fail(HD_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(rows) & 3) return fail(HD_ERR_INVALID, "rows must be 4-byte aligned");
    for (uint32_t r = 0; r < n_rows; ++r)
        if (segments[r] < 1 || segments[r] > hd::kWaterfallMaxSeg) return fail(HD_ERR_INVALID, "segments[r] must be 1..64");
    std::lock_guard<std::recursive_mutex> lock(wf->feed.e->mtx);
    if (const int rc = enter(wf->feed.e)) return rc;
    if (!n_rows) return HD_OK;
    if (device && !is_device_pointer(rows)) return fail(HD_ERR_INVALID, "rows pointer is not device memory (device = 0 takes host memory)");
    hipStream_t q = wf->feed.q;
    uint64_t first[hd_waterfall::kChunkRows];
    for (uint32_t r = 0; r < n_rows;) {
        const uint32_t slot = (uint32_t)(wf->headers.size() % wf->par.rows_cap);
        const uint32_t n = std::min(n_rows - r, std::min<uint32_t>(wf->chunk_rows, wf->par.rows_cap - slot));
        HD_HIP(hipMemcpyAsync(wf->ring.p + (size_t)slot * hd::kWaterfallBins, rows + (size_t)r * hd::kWaterfallBins, (size_t)n * hd::kWaterfallBins * sizeof(float),
                              device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, q));
        HD_HIP(hipMemcpyAsync(wf->d_seg.p, segments + r, n * sizeof(uint32_t), hipMemcpyHostToDevice, q));
        uint64_t at = wf->samples;
        for (uint32_t b = 0; b < n; ++b) { first[b] = at; at += (uint64_t)segments[r + b] * hd::kSurveyHop; }
        if (const int rc = waterfall_detect_chunk(wf, slot, n, wf->d_seg.p, 0, 0, first, segments + r)) return rc;
        wf->samples = at;
        r += n;
    }
    return HD_OK;
}

uint64_t hd_waterfall_rows_total(hd_waterfall* wf)
{
    if (!wf) return 0;
    std::lock_guard<std::recursive_mutex> lock(wf->feed.e->mtx);
    return wf->headers.size();
}

int hd_waterfall_headers(hd_waterfall* wf, uint64_t first_row, uint32_t n, hd_waterfall_row* out)
{
    if (!wf) return fail(HD_ERR_INVALID, "null waterfall");
    if (n && !out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(wf->feed.e->mtx);
    if (first_row > wf->headers.size() || n > wf->headers.size() - first_row) return fail(HD_ERR_INVALID, "rows outside [0, hd_waterfall_rows_total)");
    if (n) std::memcpy(out, wf->headers.data() + first_row, (size_t)n * sizeof(hd_waterfall_row));
    return HD_OK;
}

int hd_waterfall_marks(hd_waterfall* wf, uint64_t first_row, uint32_t n, uint32_t* out)
{
    if (!wf) return fail(HD_ERR_INVALID, "null waterfall");
    if (n && !out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(wf->feed.e->mtx);
    if (first_row > wf->headers.size() || n > wf->headers.size() - first_row) return fail(HD_ERR_INVALID, "rows outside [0, hd_waterfall_rows_total)");
    if (n) std::memcpy(out, wf->marks.data() + first_row * hd::kWaterfallWords, (size_t)n * hd::kWaterfallWords * sizeof(uint32_t));
    return HD_OK;
}

int hd_waterfall_rows(hd_waterfall* wf, uint64_t first_row, uint32_t n, float* out)
{
    if (!wf) return fail(HD_ERR_INVALID, "null waterfall");
    if (n && !out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(wf->feed.e->mtx);
    if (const int rc = enter(wf->feed.e)) return rc;
    const uint64_t total = wf->headers.size(), cap = wf->par.rows_cap;
    if (first_row > total || n > total - first_row) return fail(HD_ERR_INVALID, "rows outside [0, hd_waterfall_rows_total)");
    if (n && first_row + cap < total) return fail(HD_ERR_INVALID, "the first of these rows has left the ring (rows_cap = " + std::to_string(cap) + ")");
    for (uint32_t r = 0; r < n;) {           // at most two pieces: the ring wraps once inside rows_cap rows
        const uint32_t slot = (uint32_t)((first_row + r) % cap);
        const uint32_t k = (uint32_t)std::min<uint64_t>(n - r, cap - slot);
        HD_HIP(hipMemcpyAsync(out + (size_t)r * hd::kWaterfallBins, wf->ring.p + (size_t)slot * hd::kWaterfallBins, (size_t)k * hd::kWaterfallBins * sizeof(float),
                              hipMemcpyDeviceToHost, wf->feed.q));
        r += k;
    }
    HD_HIP(hipStreamSynchronize(wf->feed.q));
    return HD_OK;
}

int hd_waterfall_hits(hd_waterfall* wf, uint32_t hits[4096], uint64_t* rows_counted)
{
    if (!wf) return fail(HD_ERR_INVALID, "null waterfall");
    if (!hits) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(wf->feed.e->mtx);
    if (const int rc = enter(wf->feed.e)) return rc;
    HD_HIP(hipMemcpyAsync(wf->h_hits, wf->hits.p, hd::kWaterfallBins * sizeof(uint32_t), hipMemcpyDeviceToHost, wf->feed.q));
    HD_HIP(hipStreamSynchronize(wf->feed.q));
    std::memcpy(hits, wf->h_hits, hd::kWaterfallBins * sizeof(uint32_t));
    if (rows_counted) *rows_counted = wf->rows_counted;
    return HD_OK;
}

int hd_waterfall_tracks(hd_waterfall* wf, const hd_waterfall_track_params* p, hd_waterfall_track* out, uint32_t cap, uint32_t* found)
{
    if (found) *found = 0;
    if (!wf) return fail(HD_ERR_INVALID, "null waterfall");
    if (!found || (cap && !out)) return fail(HD_ERR_INVALID, "null argument");
    hd_waterfall_track_params def;
    hd::waterfall_track_params_default(&def);
    std::lock_guard<std::recursive_mutex> lock(wf->feed.e->mtx);
    if (hd::waterfall_tracks(wf->headers.data(), wf->marks.data(), wf->headers.size(), wf->feed.e->fs, p ? p : &def, out, cap, found))
        return fail(HD_ERR_INVALID, "hd_waterfall_tracks: merge_hz and max_width_hz must be >= 0");
    return HD_OK;
}

}  // extern "C"
