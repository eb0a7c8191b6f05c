// The objects that read the streams' signal beside the decode pipeline: the baud-rate probe (kernels/baud_probe.hip, host/baud_probe.hpp) and the clocked
// decoder (kernels/clocked.hip, host/clocked.hpp), which read the discriminator output, and the tone-filter demodulator (kernels/tones.hip,
// host/tones.hpp), which reads the decimated IQ and writes a row the other two can take, and the tone search (kernels/tone_search.hip,
// host/tone_search.hpp), which reads the decimated IQ too and keeps a long-averaged spectrum per stream.  All take one row per stream through the same
// three doors -- the engine's last call, rows in device memory, rows in host memory -- describe them to their kernel in a pinned array of per-stream
// descriptors, launch on the engine's first queue and wait for it.  They differ in the descriptor (launch.h: ProbeSrc, ClockedSrc, TonesSrc;
// tone_search.h: ToneSearchSrc), in the rows' element (float, or float2 for cf32) and in what they launch; the rest is the helpers below: the doors'
// checks (check_object), the three push doors and the timed one (push_engine, push_rows, push_timed), the launches of a push (launch_chunks; the probe's is
// a single one, probe_launch), the refusal of a row above max_push (check_max_push), reset and destroy, and the test hooks' guard counter.  Device memory
// is held in DevBuf and, where the kernels' rows lie between guard words, Guarded (engine_state.h): no object frees anything by hand.  Where an
// object does something of its own, it says so at its own *_launch or door.  The diversity combiner (kernels/combine.hip, host/combine.hpp) is the fifth: it
// reads float rows as the clocked decoder does (CombineSrc has ClockedSrc's fields), sums the rows of a group of streams and writes rows as the tones do.
// The SSDV object (kernels/ssdv.hip, host/ssdv.hpp) is the sixth: it takes bytes, not rows -- its doors append on the host -- and shares the doors' checks,
// the chunked launches (its descriptors' n_total counts candidates), reset, destroy and the guard counter.  The 4FSK modem (kernels/fsk4.hip,
// host/fsk4.hpp) is the seventh: the tones' doors, descriptor and chunked slot launches in front, the SSDV object's chunked candidate launches and host
// delivery behind.  The 4FSK tone tracker (kernels/fsk4_track.hip, host/fsk4_track.hpp) is the eighth: the tone search's doors, descriptor and kernel over
// accumulators of its own, cut into rounds at every stream's epoch end (launch_rounds, which the modem's retunes use too), the comb detector behind them.
// The AFSK / AX.25 modem (kernels/afsk.hip, host/afsk.hpp) is the ninth: the clocked decoder's doors and descriptor, the 4FSK modem's chunked slot
// launches, a gate launch that lists the flags, and chunked candidate launches whose records come back at places the host gave them.
#include <atomic>
#include <chrono>
#include <cstddef>

#include "engine_state.h"
#include "host/afsk.hpp"
#include "host/baud_probe.hpp"
#include "host/clocked.hpp"
#include "host/combine.hpp"
#include "host/fsk4.hpp"
#include "host/fsk4_track.hpp"
#include "host/ssdv.hpp"
#include "host/tones.hpp"
#include "host/tone_search.hpp"
#include "kernels/afsk.h"
#include "kernels/combine.h"
#include "kernels/fsk4.h"
#include "kernels/fsk4_track.h"
#include "kernels/ssdv.h"
#include "kernels/tone_search.h"

using hd::eng::enter;
using hd::eng::is_device_pointer;

namespace {

// A row's length in its descriptor.  (The clocked decoder's n is the part of the row one launch takes: clocked_launch.)
uint32_t& src_len(hd::ProbeSrc& d) { return d.n; }
uint32_t& src_len(hd::ClockedSrc& d) { return d.n_total; }
uint32_t& src_len(hd::CombineSrc& d) { return d.n_total; }

// A descriptor for n elements in linear memory at p.
template <typename Src>
void src_set(Src& d, const float* p, uint32_t n) { src_len(d) = n; d.p = p; d.sym = nullptr; d.ring_mask = 0; }
template <typename Src>
void src_set(Src& d, const float2* p, uint32_t n) { d.n_total = n; d.p = p; }            // the cf32 descriptors: TonesSrc, ToneSearchSrc

// A descriptor for what the engine's last call left for stream s, and that row's length: what hd_stream_demodulated knows -- the linear demod row, or the
// newest last_m samples of the symbol ring -- or, for the tones, what hd_stream_decimated knows.
template <typename Src>
uint32_t src_from_engine(hd_engine* e, uint32_t s, Src& d)
{
    const SizeState& sz = e->mirror[s];
    src_len(d) = sz.last_m;
    if (sz.demod_in_ring) { d.p = e->tail.p + (size_t)s * e->tail_cap; d.sym = e->d_symstate.p + s; d.ring_mask = e->tail_cap - 1u; }
    else { d.p = e->demod.p + (size_t)s * (e->demod.n / e->S); d.sym = nullptr; d.ring_mask = 0; }
    return sz.last_m;
}
template <typename Src>
uint32_t src_from_engine_iq(hd_engine* e, uint32_t s, Src& d)
{
    const SizeState& sz = e->mirror[s];
    src_set(d, e->fbuf[sz.last_buf].p + (size_t)s * e->fbuf_stride + e->fir_hist_cap + sz.last_pend_before, sz.last_n2);
    return sz.last_n2;
}
uint32_t src_from_engine(hd_engine* e, uint32_t s, hd::TonesSrc& d) { return src_from_engine_iq(e, s, d); }
uint32_t src_from_engine(hd_engine* e, uint32_t s, hd::ToneSearchSrc& d) { return src_from_engine_iq(e, s, d); }

// The helpers take any of the objects: all carry e, S, src (PinBuf of the descriptors), slab (DevBuf), pushed_calls and t0 / t1 under these names, and
// kNull, the doors' message for a null object.

// What every door that names a stream tests first, in this order: the object, then the stream's range (all: UINT32_MAX, every stream, passes too).
// Null outputs and capacities come behind it, then the lock and enter().
template <typename Obj>
int check_object(Obj* o, uint32_t stream, bool all = false)
{
    if (!o) return fail(HD_ERR_INVALID, Obj::kNull);
    if (!(all && stream == UINT32_MAX) && stream >= o->S) return fail(HD_ERR_INVALID, "stream index out of range");
    return HD_OK;
}

// hd_*_push_engine.  fn: the door's name for the message.  launch(o, max_n): the descriptors are written and the longest row has max_n samples.
template <typename Obj, typename Launch>
int push_engine(Obj* o, const char* fn, Launch launch)
{
    if (!o) return fail(HD_ERR_INVALID, Obj::kNull);
    hd_engine* e = o->e;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    if (const int rc = enter(e)) return rc;
    if (e->in_callback) return fail(HD_ERR_INVALID, std::string(fn) + " cannot be called from a sentence / character callback");
    if (const int rc = flush_locked(e)) return rc;                     // like the data getters: the call in flight is delivered first
    if (e->device_failed) return hd::eng::failed_state(e);            // (the delivery may have found the give-up word set)
    if (e->calls == o->pushed_calls) return HD_OK;                     // no call since the last push
    o->pushed_calls = e->calls;
    uint32_t max_n = 0;
    for (uint32_t s = 0; s < e->S; ++s) max_n = std::max(max_n, src_from_engine(e, s, o->src.p[s]));
    return launch(o, max_n);
}

// hd_*_push_device (device = true: row s is read in place at rows + s * stride) and hd_*_push_host (the rows are packed end to end into the slab,
// grown on demand, one copy per row on the engine's first queue).  T: a row's element, float or float2.
template <typename Obj, typename T, typename Launch>
int push_rows(Obj* o, const T* rows, size_t stride, const uint32_t* n_per_stream, uint32_t n, bool device, Launch launch)
{
    if (!o) return fail(HD_ERR_INVALID, Obj::kNull);
    if (!rows) return fail(HD_ERR_INVALID, "null rows");
    if (reinterpret_cast<uintptr_t>(rows) & (alignof(T) - 1)) return fail(HD_ERR_INVALID, "rows must be " + std::to_string(alignof(T)) + "-byte aligned");
    uint32_t max_n = 0; size_t total = 0;
    for (uint32_t s = 0; s < o->S; ++s) {
        const uint32_t ns = n_per_stream ? n_per_stream[s] : n;
        max_n = std::max(max_n, ns); total += ns;
    }
    if (o->S > 1 && max_n > stride) return fail(HD_ERR_INVALID, "a row is longer than the stride");
    std::lock_guard<std::recursive_mutex> lock(o->e->mtx);
    if (const int rc = enter(o->e)) return rc;
    if (!total) return HD_OK;                  // nothing to read: before the device-pointer check
    if (device && !is_device_pointer(rows)) return fail(HD_ERR_INVALID, "rows are not device memory (the _host call takes host memory)");
    if (!device) HD_HIP(o->slab.grow(total));
    size_t at = 0;
    for (uint32_t s = 0; s < o->S; ++s) {
        auto& d = o->src.p[s];
        const uint32_t ns = n_per_stream ? n_per_stream[s] : n;
        src_set(d, device ? rows + (size_t)s * stride : o->slab.p + at, ns);
        if (!device && ns) HD_HIP(hipMemcpyAsync(o->slab.p + at, rows + (size_t)s * stride, (size_t)ns * sizeof(T), hipMemcpyHostToDevice, o->e->qa));
        at += ns;
    }
    return launch(o, max_n);
}

// The launches behind a push of the clocked decoder, the tones and the tone search: src[s].p and n_total are written and the longest row has max_n samples;
// one launch per `chunk` samples of it, each waited for before the next one's descriptors are written.  Chunk by chunk: every descriptor's off and n are
// cut from its n_total, and prepare(s, d) adds, in the same pass over the streams (a second pass is host time a push of 1024 streams shows), what the
// object's kernel wants beside them; launch() issues the kernel -- false: it does not fit, the push fails with `unfit` -- and starts the object's
// per-chunk maxima afresh; after() follows the wait.  t1 is recorded behind the last chunk's launch.  (The probe's kernel takes a row whole: probe_launch.)
template <typename Obj, typename Prepare, typename Launch, typename After>
int launch_chunks(Obj* o, uint32_t max_n, uint32_t chunk, const char* unfit, Prepare prepare, Launch launch, After after)
{
    hipStream_t q = o->e->qa;
    if (o->t0) HD_HIP(hipEventRecord(o->t0, q));
    for (uint32_t off = 0; off < max_n; off += chunk) {
        for (uint32_t s = 0; s < o->S; ++s) {
            auto& d = o->src.p[s];
            d.off = off;
            d.n = d.n_total > off ? std::min<uint32_t>(chunk, d.n_total - off) : 0u;
            prepare(s, d);
        }
        std::atomic_thread_fence(std::memory_order_release);
        if (!launch()) return fail(HD_ERR_DEVICE, unfit);
        HD_HIP(hipGetLastError());
        if (o->t1 && off + chunk >= max_n) HD_HIP(hipEventRecord(o->t1, q));
        HD_HIP(hipStreamSynchronize(q));
        after();
    }
    return HD_OK;
}

// The launches behind a push whose streams are cut each at places of its own -- the tracker's epoch ends, the 4FSK modem's retunes: round by round,
// take(s, d, left) says how many of the `left` samples stream s still has the next launch takes (at least one; d.off and d.n are written here, the
// rest of the descriptor by take), launch() issues the kernel (false: it does not fit, the push fails with `unfit`), after() follows the wait and may
// launch and wait for more.  Without cuts the rounds are launch_chunks' chunks.  o->done [S]: the object's scratch.  A stream with nothing left is
// not asked: its descriptor gets n = 0 and keeps whatever else an earlier round wrote there, which no kernel reads -- k_tone_search and k_fsk4_slots
// leave at n = 0 before they look at another field.
template <typename Obj, typename Take, typename Launch, typename After>
int launch_rounds(Obj* o, const char* unfit, Take take, Launch launch, After after)
{
    hipStream_t q = o->e->qa;
    if (o->t0) HD_HIP(hipEventRecord(o->t0, q));
    o->done.assign(o->S, 0u);
    for (;;) {
        bool any = false;
        for (uint32_t s = 0; s < o->S; ++s) {
            auto& d = o->src.p[s];
            const uint32_t left = d.n_total - o->done[s];
            d.off = o->done[s];
            d.n = left ? take(s, d, left) : 0u;
            o->done[s] += d.n;
            any |= d.n != 0;
        }
        if (!any) break;
        std::atomic_thread_fence(std::memory_order_release);
        if (!launch()) return fail(HD_ERR_DEVICE, unfit);
        HD_HIP(hipGetLastError());
        if (o->t1) HD_HIP(hipEventRecord(o->t1, q));                   // (recorded again behind every launch: the last one's stands)
        HD_HIP(hipStreamSynchronize(q));
        if (const int rc = after()) return rc;
    }
    return HD_OK;
}

// Tones and tone search: a row above max_push refuses the whole push, before t0 is recorded and anything is launched.  first(s) goes in front of
// stream s's test, in the same pass: the tones pass a stream without a modem by there.  max_n: the longest row, counted again behind that.
template <typename Obj, typename First>
int check_max_push(Obj* o, const char* who, uint32_t* max_n, First first)
{
    *max_n = 0;
    for (uint32_t s = 0; s < o->S; ++s) {
        first(s);
        const uint32_t n = o->src.p[s].n_total;
        if (n > o->prm.max_push)
            return fail(HD_ERR_CAPACITY, std::string(who) + ": a push of " + std::to_string(n) + " samples, max_push is " + std::to_string(o->prm.max_push));
        *max_n = std::max(*max_n, n);
    }
    return HD_OK;
}

// The measurement hooks (tools/micro/*_rate.py; not part of the ABI): the kernels of push() -- the object's hd_*_push_engine, whose
// launch records t0 and t1 where they are set -- between two HIP events, and the host time of the whole call in microseconds.
template <typename Obj, typename Push>
int push_timed(Obj* o, float* kernel_ms, double* host_us, Push push)
{
    if (!o || !kernel_ms || !host_us) return fail(HD_ERR_INVALID, "null argument");
    hd_engine* e = o->e;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    if (const int rc = enter(e)) return rc;
    if (const int rc = flush_locked(e)) return rc;
    HD_HIP(hipEventCreate(&o->t0));
    HD_HIP(hipEventCreate(&o->t1));
    const uint64_t before = o->pushed_calls;
    const auto w0 = std::chrono::steady_clock::now();
    const int rc = push(o);
    *host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
    *kernel_ms = 0;
    if (rc == HD_OK && o->pushed_calls != before && hipEventQuery(o->t1) == hipSuccess) (void)hipEventElapsedTime(kernel_ms, o->t0, o->t1);
    (void)hipGetLastError();
    (void)hipEventDestroy(o->t0); (void)hipEventDestroy(o->t1);
    o->t0 = o->t1 = nullptr;
    return rc;
}

// hd_*_reset.  clear(o, s0, ns): the object's own, streams s0 .. s0 + ns - 1 go back to their modem's first state.
template <typename Obj, typename Clear>
int reset(Obj* o, uint32_t stream, Clear clear)
{
    if (const int rc = check_object(o, stream, true)) return rc;
    std::lock_guard<std::recursive_mutex> lock(o->e->mtx);
    if (const int rc = enter(o->e)) return rc;
    return stream == UINT32_MAX ? clear(o, 0, o->S) : clear(o, stream, 1);
}

// The test hooks hd_debug_*_guards (not part of the ABI): how many guard words in front of and behind each of the rows no longer hold their array's
// pattern.  Which rows an object guards is its own list; where a row's guards lie, how wide they are and what they hold is its array's (Guarded).
int damaged_guards(std::initializer_list<GuardedRow> rows)
{
    std::vector<uint32_t> g;
    int bad = 0;
    for (const GuardedRow& r : rows)
        for (const uint32_t* p : {r.front, r.back}) {
            g.resize(r.G);
            HD_HIP(hipMemcpy(g.data(), p, r.G * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint32_t w : g) bad += w != r.pattern;
        }
    return bad;
}

// hd_*_create of the objects that write or refuse by max_push: 0 is the default, what the engine's longest call leaves or 4096; above 2^28 it is refused.
// who: the object in the message.
int default_max_push(const hd_engine* e, uint32_t* max_push, const char* who)
{
    if (!*max_push) *max_push = std::max<uint32_t>(e->n2_cap, 4096u);
    if (*max_push > (1u << 28)) return fail(HD_ERR_INVALID, std::string(who) + " parameters: max_push <= 2^28");
    return HD_OK;
}

// hd_tones_rows / hd_combine_rows: the rows the object's last push wrote, in place.  Both objects carry them as rows (Guarded<float>) and row_n.
template <typename Obj>
int output_rows(Obj* o, const float** d_rows, size_t* stride, uint32_t* n_per_stream)
{
    if (!o) return fail(HD_ERR_INVALID, Obj::kNull);
    if (!d_rows || !stride || !n_per_stream) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(o->e->mtx);
    *d_rows = o->rows.row(0);
    *stride = o->rows.stride;
    std::memcpy(n_per_stream, o->row_n.data(), (size_t)o->S * sizeof(uint32_t));
    return HD_OK;
}

// hd_tones_output / hd_combine_output: one of those rows to the host; returns its length, whatever cap let through.
template <typename Obj>
int output_row(Obj* o, uint32_t stream, float* out, size_t cap)
{
    if (const int rc = check_object(o, stream)) return rc;
    if (cap && !out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(o->e->mtx);
    if (const int rc = enter(o->e)) return rc;
    const size_t k = std::min<size_t>(o->row_n[stream], cap);
    if (k) HD_HIP(hipMemcpy(out, o->rows.row(stream), k * sizeof(float), hipMemcpyDeviceToHost));
    return (int)o->row_n[stream];
}

// hd_*_destroy.  (No queue to wait for: every push has waited for its launches.)
template <typename Obj>
void destroy(Obj* o)
{
    if (!o) return;
    hd_engine* e = o->e;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    (void)hipSetDevice(e->cfg.device);
    delete o;
}

}  // namespace

/* ---------------------------------------------------------------- baud-rate probe (kernels/baud_probe.hip) ----------------------------- */

struct hd_baud_probe {
    static constexpr const char* kNull = "null probe";
    hd_engine* e = nullptr;
    hd_baud_probe_params prm{};
    hd::BaudProbeTables t;
    uint32_t S = 0;
    DevBuf<hd_baud_probe_stream_state> hdr;      // [S]
    DevBuf<unsigned long long> acc64;            // [S][2][1024]: P, Q
    DevBuf<uint32_t> acc32;                      // [S][5][1024]: NB, re, im, n, cur_block
    DevBuf<uint32_t> F, scale;
    DevBuf<int32_t> ctab;
    DevBuf<float> slab;                          // hd_baud_probe_push_host: the rows packed end to end, grown on demand
    PinBuf<hd::ProbeSrc> src;                    // [S]: the push's descriptors, read by the kernel in place (a push returns when its kernel is done)
    uint64_t pushed_calls = 0;                   // hd_baud_probe_push_engine: e->calls at the last push (the call delivered last is calls - 1)
    hipEvent_t t0 = nullptr, t1 = nullptr;       // set by the measurement hook only: recorded around the launch
};

namespace {

// The descriptors are written: one launch for all streams on the engine's first queue, and the wait for it.  Its own: the kernel takes a row whole, so
// there is no chunk loop, and nothing is launched when every stream's row is empty (hd_baud_probe_push_engine; the other doors return before that).
int probe_launch(hd_baud_probe* p, uint32_t max_n)
{
    if (!max_n) return HD_OK;
    std::atomic_thread_fence(std::memory_order_release);
    if (p->t0) HD_HIP(hipEventRecord(p->t0, p->e->qa));
    hd::launch_baud_probe(p->e->qa, p->S, p->src.dev, p->hdr.p, p->acc64.p, p->acc32.p, p->F.p, p->scale.p, p->ctab.p);
    if (p->t1) HD_HIP(hipEventRecord(p->t1, p->e->qa));
    HD_HIP(hipGetLastError());
    HD_HIP(hipStreamSynchronize(p->e->qa));
    return HD_OK;
}

int probe_clear(hd_baud_probe* p, uint32_t s0, uint32_t ns)
{
    hipStream_t q = p->e->qa;
    HD_HIP(hipMemsetAsync(p->hdr.p + s0, 0, (size_t)ns * sizeof(hd_baud_probe_stream_state), q));
    HD_HIP(hipMemsetAsync(p->acc64.p + (size_t)s0 * 2 * hd::kProbeCand, 0, (size_t)ns * 2 * hd::kProbeCand * sizeof(unsigned long long), q));
    HD_HIP(hipMemsetAsync(p->acc32.p + (size_t)s0 * 5 * hd::kProbeCand, 0, (size_t)ns * 5 * hd::kProbeCand * sizeof(uint32_t), q));
    HD_HIP(hipStreamSynchronize(q));
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_baud_probe_params_default(hd_baud_probe_params* p) { if (p) hd::baud_probe_params_default(p); }

int hd_baud_probe_create(hd_engine* e, const hd_baud_probe_params* params, hd_baud_probe** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_baud_probe> p(new hd_baud_probe);
    p->e = e; p->S = e->S;
    hd::baud_probe_params_default(&p->prm);
    if (params) p->prm = *params;
    if (!hd::baud_probe_params_ok(&p->prm, e->fsd))
        return fail(HD_ERR_INVALID, "baud probe parameters: 0 < baud_lo < baud_hi <= decimated rate / 3.5 (" + std::to_string(e->fsd / 3.5) + ") and min_coherence >= 0");
    if (const int rc = enter(e)) return rc;
    p->t.make(e->fsd, p->prm);
    std::vector<uint32_t> sc(hd::kProbeCand);
    for (uint32_t k = 0; k < hd::kProbeCand; ++k) sc[k] = p->t.scale[k];
    HD_HIP(p->hdr.alloc_unfilled(p->S));
    HD_HIP(p->acc64.alloc_unfilled((size_t)p->S * 2 * hd::kProbeCand));
    HD_HIP(p->acc32.alloc_unfilled((size_t)p->S * 5 * hd::kProbeCand));
    HD_HIP(p->F.alloc_unfilled(hd::kProbeCand));
    HD_HIP(p->scale.alloc_unfilled(hd::kProbeCand));
    HD_HIP(p->ctab.alloc_unfilled(1024));
    HD_HIP(p->src.alloc(p->S));
    HD_HIP(hipMemcpyAsync(p->F.p, p->t.F, hd::kProbeCand * sizeof(uint32_t), hipMemcpyHostToDevice, e->qa));
    HD_HIP(hipMemcpyAsync(p->scale.p, sc.data(), hd::kProbeCand * sizeof(uint32_t), hipMemcpyHostToDevice, e->qa));
    HD_HIP(hipMemcpyAsync(p->ctab.p, p->t.C, 1024 * sizeof(int32_t), hipMemcpyHostToDevice, e->qa));
    if (const int rc = probe_clear(p.get(), 0, p->S)) return rc;       // (waits for the queue: `sc` is a local)
    p->pushed_calls = 0;
    *out = p.release();
    return HD_OK;
}

void hd_baud_probe_destroy(hd_baud_probe* p) { destroy(p); }

int hd_baud_probe_reset(hd_baud_probe* p, uint32_t stream) { return reset(p, stream, probe_clear); }

int hd_baud_probe_push_engine(hd_baud_probe* p) { return push_engine(p, "hd_baud_probe_push_engine", probe_launch); }

int hd_baud_probe_push_device(hd_baud_probe* p, const float* d_rows, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(p, d_rows, stride, n_per_stream, n, true, probe_launch);
}

int hd_baud_probe_push_host(hd_baud_probe* p, const float* rows, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(p, rows, stride, n_per_stream, n, false, probe_launch);
}

int hd_baud_probe_state(hd_baud_probe* p, uint32_t stream, hd_baud_probe_stream_state* hdr, hd_baud_probe_candidate* cand, size_t cap)
{
    if (const int rc = check_object(p, stream)) return rc;
    if (cap < hd::kProbeCand) return (int)hd::kProbeCand;              // nothing is written
    std::lock_guard<std::recursive_mutex> lock(p->e->mtx);
    if (const int rc = enter(p->e)) return rc;
    hd_baud_probe_stream_state h;
    std::vector<unsigned long long> a64(2 * hd::kProbeCand);
    std::vector<uint32_t> a32(5 * hd::kProbeCand);
    HD_HIP(hipMemcpy(&h, p->hdr.p + stream, sizeof h, hipMemcpyDeviceToHost));
    HD_HIP(hipMemcpy(a64.data(), p->acc64.p + (size_t)stream * a64.size(), a64.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HD_HIP(hipMemcpy(a32.data(), p->acc32.p + (size_t)stream * a32.size(), a32.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    h.n_candidates = hd::kProbeCand;
    if (hdr) *hdr = h;
    for (uint32_t k = 0; cand && k < hd::kProbeCand; ++k) {
        hd_baud_probe_candidate& c = cand[k];
        c.P = a64[k]; c.Q = a64[hd::kProbeCand + k];
        c.NB = a32[k]; c.re = (int32_t)a32[hd::kProbeCand + k]; c.im = (int32_t)a32[2 * hd::kProbeCand + k];
        c.n = a32[3 * hd::kProbeCand + k]; c.cur_block = a32[4 * hd::kProbeCand + k]; c._pad = 0;
    }
    return (int)hd::kProbeCand;
}

int hd_baud_probe_estimate(hd_baud_probe* p, uint32_t stream, hd_baud_estimate* out)
{
    if (!p) return fail(HD_ERR_INVALID, hd_baud_probe::kNull);
    if (!out) return fail(HD_ERR_INVALID, "null output");                // (in front of the stream's range here: hd_baud_probe_state tests that)
    hd_baud_probe_stream_state h;
    std::vector<hd_baud_probe_candidate> c(hd::kProbeCand);
    const int n = hd_baud_probe_state(p, stream, &h, c.data(), c.size());
    if (n < 0) return n;
    hd::baud_probe_estimate(p->t, p->prm, h, c.data(), out);
    return HD_OK;
}

int hd_debug_baud_probe_push_timed(hd_baud_probe* p, float* kernel_ms, double* host_us) { return push_timed(p, kernel_ms, host_us, hd_baud_probe_push_engine); }

}  // extern "C"

/* ---------------------------------------------------------------- clocked decoder (kernels/clocked.hip) -------------------------------- */

struct hd_clocked {
    static constexpr const char* kNull = "null clocked decoder";
    hd_engine* e = nullptr;
    hd_clocked_params prm{};
    uint32_t S = 0;
    DevBuf<hd::ClockedState> st;                 // [S]
    Guarded<uint32_t> ring;                      // [S]: guard | HD_CLOCKED_RING running sums | guard
    Guarded<uint32_t> rec;                       // [S]: guard | record_cap records | guard
    DevBuf<float> slab;                          // hd_clocked_push_host: the rows packed end to end, grown on demand
    PinBuf<hd::ClockedSrc> src;                  // [S]: a launch's descriptors, read by the kernel in place (a launch is waited for before the next is written)
    std::vector<hd::ClockedState> modem;         // [S]: the state a reset gives the stream (F = 0: off)
    std::vector<hd::ClockedText> tx;             // [S]
    uint64_t pushed_calls = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;       // set by the measurement hook only: recorded around the launches of a push
};
// (the strides the kernel was written against, launch.h)
static_assert(Guarded<uint32_t>::stride_of(HD_CLOCKED_RING, hd::kClockedGuard) == HD_CLOCKED_RING + 2 * hd::kClockedGuard, "clocked ring stride");
static_assert(Guarded<uint32_t>::stride_of(1024 * hd::kClockedRecWords, hd::kClockedGuard) == 1024 * hd::kClockedRecWords + 2 * hd::kClockedGuard, "clocked record stride");

namespace {

// Its own per chunk: the LDS window of the launch, the widest any stream with a modem needs for its part of the row.
int clocked_launch(hd_clocked* c, uint32_t max_n)
{
    uint32_t lds_words = 64;
    return launch_chunks(
        c, max_n, HD_CLOCKED_CHUNK, "clocked decoder: the launch's window does not fit the LDS",
        [&](uint32_t s, const hd::ClockedSrc& d) {
            if (c->modem[s].F) lds_words = std::max(lds_words, hd::clocked_window_words(c->modem[s], d.n));
        },
        [&] {
            const uint32_t words = lds_words;
            lds_words = 64;
            return hd::launch_clocked(c->e->qa, c->S, c->src.dev, c->st.p, c->ring.base(), c->ring.stride, c->rec.base(), c->rec.stride, c->prm.record_cap, words);
        },
        [] {});
}

int clocked_clear(hd_clocked* c, uint32_t s0, uint32_t ns)
{
    hipStream_t q = c->e->qa;
    HD_HIP(hipMemcpyAsync(c->st.p + s0, c->modem.data() + s0, (size_t)ns * sizeof(hd::ClockedState), hipMemcpyHostToDevice, q));
    HD_HIP(hipMemset2DAsync(c->ring.row(s0), c->ring.stride * sizeof(uint32_t), 0,
                            (size_t)HD_CLOCKED_RING * sizeof(uint32_t), ns, q));
    HD_HIP(hipStreamSynchronize(q));
    for (uint32_t s = s0; s < s0 + ns; ++s) { c->tx[s].reset(); c->tx[s].nbits = c->modem[s].nbits; }
    return HD_OK;
}

// The stream's waiting records leave the ring through its text stage; up to cap of them are copied to out (out null: none are kept).
int clocked_drain(hd_clocked* c, uint32_t s, hd_clocked_record* out, size_t cap, size_t* n_out)
{
    hd::ClockedState h;
    HD_HIP(hipMemcpy(&h, c->st.p + s, sizeof h, hipMemcpyDeviceToHost));
    const uint64_t have = h.written - h.taken, rc = c->prm.record_cap;
    const size_t k = out ? (size_t)std::min<uint64_t>(have, cap) : (size_t)have;
    *n_out = k;
    if (!k) return HD_OK;
    std::vector<hd_clocked_record> tmp(k);
    const uint32_t* base = c->rec.row(s);
    for (size_t i = 0; i < k;) {             // at most two pieces: the ring wraps once inside record_cap records
        const uint64_t slot = (h.taken + i) % rc;
        const size_t m = (size_t)std::min<uint64_t>(k - i, rc - slot);
        HD_HIP(hipMemcpy(tmp.data() + i, base + slot * hd::kClockedRecWords, m * sizeof(hd_clocked_record), hipMemcpyDeviceToHost));
        i += m;
    }
    h.taken += k;
    HD_HIP(hipMemcpy(reinterpret_cast<char*>(c->st.p + s) + offsetof(hd::ClockedState, taken), &h.taken, sizeof h.taken, hipMemcpyHostToDevice));
    c->tx[s].feed(tmp.data(), k);
    if (out) std::memcpy(out, tmp.data(), k * sizeof(hd_clocked_record));
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_clocked_params_default(hd_clocked_params* p) { if (p) hd::clocked_params_default(p); }

int hd_clocked_create(hd_engine* e, const hd_clocked_params* params, hd_clocked** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_clocked> c(new hd_clocked);
    c->e = e; c->S = e->S;
    hd::clocked_params_default(&c->prm);
    if (params) c->prm = *params;
    if (!hd::clocked_params_ok(&c->prm)) return fail(HD_ERR_INVALID, "clocked decoder parameters: 16 <= record_cap <= 2^20, repair_bits <= 16, repair_flips <= 4");
    if (const int rc = enter(e)) return rc;
    c->modem.resize(c->S);
    c->tx.resize(c->S);
    for (uint32_t s = 0; s < c->S; ++s) {
        const uint32_t nbits = (uint32_t)e->st[s].text.framer.nbits;
        const double nstops = (double)e->st[s].text.framer.nstops;
        const uint32_t F = hd::clocked_modem_F(e->fsd, e->st[s].baud, nbits, nstops);
        hd::clocked_state_reset(c->modem[s], F, F ? nbits : 0u, F ? (uint32_t)nstops : 0u, 0u);
        c->tx[s].repair_bits = c->prm.repair_bits; c->tx[s].repair_flips = c->prm.repair_flips;
    }
    HD_HIP(c->st.alloc_unfilled(c->S));
    HD_HIP(c->ring.alloc(c->S, HD_CLOCKED_RING, hd::kClockedGuard, hd::kClockedGuardWord, e->qa));
    HD_HIP(c->rec.alloc(c->S, (size_t)c->prm.record_cap * hd::kClockedRecWords, hd::kClockedGuard, hd::kClockedGuardWord, e->qa));
    HD_HIP(c->src.alloc(c->S));
    if (const int rc = clocked_clear(c.get(), 0, c->S)) return rc;
    *out = c.release();
    return HD_OK;
}

void hd_clocked_destroy(hd_clocked* c) { destroy(c); }

int hd_clocked_reset(hd_clocked* c, uint32_t stream) { return reset(c, stream, clocked_clear); }

int hd_clocked_set_modem(hd_clocked* c, uint32_t stream, double baud, uint32_t nbits, uint32_t nstops, int invert)
{
    if (const int rc = check_object(c, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    const uint32_t F = hd::clocked_modem_F(c->e->fsd, baud, nbits, (double)nstops);
    if (!F) return fail(HD_ERR_UNSUPPORTED, "clocked decoder: 3.5 <= decimated rate / baud <= " + std::to_string(HD_CLOCKED_MAX_SPB) + ", 7 or 8 data bits, 1 or 2 stop bits");
    if (const int rc = enter(c->e)) return rc;
    hd::clocked_state_reset(c->modem[stream], F, nbits, nstops, invert ? 1u : 0u);
    return clocked_clear(c, stream, 1);
}

int hd_clocked_push_engine(hd_clocked* c) { return push_engine(c, "hd_clocked_push_engine", clocked_launch); }

int hd_clocked_push_device(hd_clocked* c, const float* d_rows, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(c, d_rows, stride, n_per_stream, n, true, clocked_launch);
}

int hd_clocked_push_host(hd_clocked* c, const float* rows, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(c, rows, stride, n_per_stream, n, false, clocked_launch);
}

int hd_clocked_records(hd_clocked* c, uint32_t stream, hd_clocked_record* out, size_t cap)
{
    if (const int rc = check_object(c, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = enter(c->e)) return rc;
    if (!out) {
        hd::ClockedState h;
        HD_HIP(hipMemcpy(&h, c->st.p + stream, sizeof h, hipMemcpyDeviceToHost));
        return (int)(h.written - h.taken);
    }
    size_t n = 0;
    if (const int rc = clocked_drain(c, stream, out, cap, &n)) return rc;
    return (int)n;
}

int hd_clocked_take_sentences(hd_clocked* c, uint32_t stream, hd_clocked_sentence* out, size_t cap)
{
    if (const int rc = check_object(c, stream)) return rc;
    if (cap && !out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = enter(c->e)) return rc;
    size_t n = 0;
    if (const int rc = clocked_drain(c, stream, nullptr, 0, &n)) return rc;
    return (int)c->tx[stream].take(out, cap);
}

int hd_clocked_stats(hd_clocked* c, uint32_t stream, hd_clocked_counters* out)
{
    if (const int rc = check_object(c, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = enter(c->e)) return rc;
    hd::ClockedState h;
    HD_HIP(hipMemcpy(&h, c->st.p + stream, sizeof h, hipMemcpyDeviceToHost));
    const hd::ClockedText& t = c->tx[stream];
    *out = hd_clocked_counters{h.n, h.p, h.chars, h.rejects, h.dropped, t.matches_failed, t.plain, t.repaired};
    return HD_OK;
}

int hd_debug_clocked_push_timed(hd_clocked* c, float* kernel_ms, double* host_us) { return push_timed(c, kernel_ms, host_us, hd_clocked_push_engine); }

// Test hook (tests/test_gpu_clocked.py; not part of the ABI): how many of the guard words around the stream's two rings no longer hold their pattern.
int hd_debug_clocked_guards(hd_clocked* c, uint32_t stream)
{
    if (!c || stream >= c->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = enter(c->e)) return rc;
    return damaged_guards({{c->ring, stream}, {c->rec, stream}});
}

}  // extern "C"

/* ---------------------------------------------------------------- tone-filter demodulator (kernels/tones.hip) -------------------------- */

struct hd_tones {
    static constexpr const char* kNull = "null tones object";
    hd_engine* e = nullptr;
    hd_tones_params prm{};
    uint32_t S = 0;
    DevBuf<hd::TonesState> st;                   // [S]
    Guarded<uint32_t> ring32;                    // [S * 4]: guard | kTonesRing32 running sums | guard
    Guarded<unsigned long long> ring64;          // [S]: guard | kTonesRing64 running sums | guard
    DevBuf<int32_t> ctab;                        // [1024]
    Guarded<float> rows;                         // [S]: guard | max_push floats | guard
    DevBuf<float2> slab;                         // hd_tones_push_host: the rows packed end to end, grown on demand
    PinBuf<hd::TonesSrc> src;                    // [S]: a launch's descriptors, read by the kernel in place (a launch is waited for before the next is written)
    std::vector<hd::TonesState> modem;           // [S]: the state a reset gives the stream (F = 0: no modem)
    std::vector<double> baud;                    // [S]: the engine stream's baud rate when the object was made
    std::vector<uint32_t> row_n;                 // [S]: the rows' lengths after the last push
    uint64_t pushed_calls = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;       // set by the measurement hook only: recorded around the launches of a push
};
// (the strides the kernel was written against, launch.h; the 64-bit ring's guards are kTonesGuard / 2 of its words each)
static_assert(Guarded<uint32_t>::stride_of(hd::kTonesRing32, hd::kTonesGuard) == hd::kTonesRing32 + 2 * hd::kTonesGuard, "tones 32-bit ring stride");
static_assert(Guarded<unsigned long long>::stride_of(hd::kTonesRing64, hd::kTonesGuard) == hd::kTonesRing64 + hd::kTonesGuard, "tones 64-bit ring stride");
static_assert(Guarded<float>::stride_of(4096, hd::kTonesGuard) == 4096 + 2 * hd::kTonesGuard, "tones row stride");

namespace {

// Its own: a stream without a modem is passed by, in front of the max_push test; the rows' lengths are kept for hd_tones_rows; per chunk, `cap`, the
// longest part of a row in the launch, which sizes its LDS.
int tones_launch(hd_tones* t, uint32_t max_n)
{
    if (const int rc = check_max_push(t, "hd_tones", &max_n, [t](uint32_t s) { if (!t->modem[s].F) t->src.p[s].n_total = 0; })) return rc;
    for (uint32_t s = 0; s < t->S; ++s) t->row_n[s] = t->src.p[s].n_total;
    uint32_t cap = 0;
    return launch_chunks(
        t, max_n, HD_TONES_CHUNK, "tones: the launch's chunk does not fit the LDS",
        [&](uint32_t, const hd::TonesSrc& d) { cap = std::max(cap, d.n); },
        [&] {
            const uint32_t longest = cap;
            cap = 0;
            return hd::launch_tones(t->e->qa, t->S, longest, t->src.dev, t->st.p, t->ring32.base(), t->ring32.stride, t->ring64.base(), t->ring64.stride, t->ctab.p,
                                    t->rows.base(), t->rows.stride, t->prm.max_push);
        },
        [] {});
}

// (The rings need no clearing: nothing in front of a stream's index 0 is read.)
int tones_clear(hd_tones* t, uint32_t s0, uint32_t ns)
{
    hipStream_t q = t->e->qa;
    HD_HIP(hipMemcpyAsync(t->st.p + s0, t->modem.data() + s0, (size_t)ns * sizeof(hd::TonesState), hipMemcpyHostToDevice, q));
    HD_HIP(hipStreamSynchronize(q));
    for (uint32_t s = s0; s < s0 + ns; ++s) t->row_n[s] = 0;
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_tones_params_default(hd_tones_params* p) { if (p) hd::tones_params_default(p); }

int hd_tones_create(hd_engine* e, const hd_tones_params* params, hd_tones** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_tones> t(new hd_tones);
    t->e = e; t->S = e->S;
    hd::tones_params_default(&t->prm);
    if (params) t->prm = *params;
    if (!hd::tones_window_ok(t->prm.window_q8)) return fail(HD_ERR_UNSUPPORTED, "tones parameters: 32 <= window_q8 <= 256");
    if (const int rc = default_max_push(e, &t->prm.max_push, "tones")) return rc;
    if (const int rc = enter(e)) return rc;
    t->modem.resize(t->S);
    t->baud.resize(t->S);
    t->row_n.assign(t->S, 0u);
    for (uint32_t s = 0; s < t->S; ++s) {
        hd::tones_state_reset(t->modem[s], 0, 0, 0, 0);
        t->baud[s] = e->st[s].baud;
    }
    int32_t C[1024];
    hd::tones_table(C);
    HD_HIP(t->st.alloc_unfilled(t->S));
    HD_HIP(t->ring32.alloc((size_t)t->S * 4, hd::kTonesRing32, hd::kTonesGuard, hd::kTonesGuardWord, e->qa));
    HD_HIP(t->ring64.alloc(t->S, hd::kTonesRing64, hd::kTonesGuard, hd::kTonesGuardWord, e->qa));
    HD_HIP(t->rows.alloc(t->S, t->prm.max_push, hd::kTonesGuard, hd::kTonesGuardWord, e->qa));
    HD_HIP(t->ctab.alloc_unfilled(1024));
    HD_HIP(t->src.alloc(t->S));
    HD_HIP(hipMemcpyAsync(t->ctab.p, C, sizeof C, hipMemcpyHostToDevice, e->qa));
    if (const int rc = tones_clear(t.get(), 0, t->S)) return rc;       // (waits for the queue: `C` is a local)
    *out = t.release();
    return HD_OK;
}

void hd_tones_destroy(hd_tones* t) { destroy(t); }

int hd_tones_reset(hd_tones* t, uint32_t stream) { return reset(t, stream, tones_clear); }

int hd_tones_set_modem(hd_tones* t, uint32_t stream, double baud, double f_hi_hz, double f_lo_hz)
{
    if (const int rc = check_object(t, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(t->e->mtx);
    hd::TonesState m;
    const int rc = hd::tones_modem(m, t->e->fsd, baud == 0 ? t->baud[stream] : baud, f_hi_hz, f_lo_hz, t->prm.window_q8);
    if (rc == HD_ERR_UNSUPPORTED) return fail(rc, "tones: 3.5 <= decimated rate / baud <= " + std::to_string(HD_TONES_MAX_SPB) + " and 32 <= window_q8 <= 256");
    if (rc) return fail(rc, "tones: |tone| < decimated rate / 2 and f_hi above f_lo");
    if (const int rc2 = enter(t->e)) return rc2;
    t->modem[stream] = m;
    return tones_clear(t, stream, 1);
}

int hd_tones_set_modem_from_afc(hd_tones* t, uint32_t stream, double baud)
{
    if (const int rc = check_object(t, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(t->e->mtx);
    hd_afc_info a;
    if (const int rc = hd_stream_afc(t->e, stream, &a)) return rc;
    if (a.peak_left <= 0 || a.peak_right <= 0) return fail(HD_ERR_INVALID, "tones: the stream's AFC has no two valid peaks");
    const double bin = t->e->fsd / 4096.0;
    return hd_tones_set_modem(t, stream, baud, (a.peak_right - 2048) * bin, (a.peak_left - 2048) * bin);
}

int hd_tones_push_engine(hd_tones* t) { return push_engine(t, "hd_tones_push_engine", tones_launch); }

int hd_tones_push_device(hd_tones* t, const float* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(t, reinterpret_cast<const float2*>(d_iq), stride, n_per_stream, n, true, tones_launch);
}

int hd_tones_push_host(hd_tones* t, const float* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(t, reinterpret_cast<const float2*>(iq), stride, n_per_stream, n, false, tones_launch);
}

int hd_tones_rows(hd_tones* t, const float** d_rows, size_t* stride, uint32_t* n_per_stream) { return output_rows(t, d_rows, stride, n_per_stream); }

int hd_tones_output(hd_tones* t, uint32_t stream, float* out, size_t cap) { return output_row(t, stream, out, cap); }

int hd_tones_stats(hd_tones* t, uint32_t stream, hd_tones_info* out)
{
    if (const int rc = check_object(t, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(t->e->mtx);
    if (const int rc = enter(t->e)) return rc;
    hd::TonesState h;
    HD_HIP(hipMemcpy(&h, t->st.p + stream, sizeof h, hipMemcpyDeviceToHost));
    *out = hd_tones_info{h.n, h.F, h.full, h.W, h.L, h.phi[0], h.phi[1]};
    return HD_OK;
}

int hd_debug_tones_push_timed(hd_tones* t, float* kernel_ms, double* host_us) { return push_timed(t, kernel_ms, host_us, hd_tones_push_engine); }

// Test hook (tests/test_gpu_tones.py; not part of the ABI): how many of the guard words around the stream's five rings and its row no longer hold their pattern.
int hd_debug_tones_guards(hd_tones* t, uint32_t stream)
{
    if (!t || stream >= t->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(t->e->mtx);
    if (const int rc = enter(t->e)) return rc;
    const size_t r = (size_t)stream * 4;
    return damaged_guards({{t->ring32, r}, {t->ring32, r + 1}, {t->ring32, r + 2}, {t->ring32, r + 3}, {t->ring64, stream}, {t->rows, stream}});
}

}  // extern "C"

/* ---------------------------------------------------------------- tone search (kernels/tone_search.hip) -------------------------------- */

struct hd_tone_search {
    static constexpr const char* kNull = "null tone search";
    hd_engine* e = nullptr;
    hd_tone_search_params prm{};
    uint32_t S = 0;
    Guarded<double> acc;                         // [S]: guard | 4096 fftshifted sums | guard
    Guarded<float2> carry;                       // [S * 2]: guard | 4096 samples | guard -- the stream's two carry buffers (kernels/tone_search.hip)
    DevBuf<float> win;                           // [4096] the survey's window table
    DevBuf<float2> own_tw;                       // the twiddles where the engine computes no spectra and holds none
    const float2* tw = nullptr;
    double sum_w2 = 0;                           // sum of w^2, in double over the float table
    DevBuf<float2> slab;                         // hd_tone_search_push_host: the rows packed end to end, grown on demand
    PinBuf<hd::ToneSearchSrc> src;               // [S]: a launch's descriptors, read by the kernel in place (a launch is waited for before the next is written)
    std::vector<uint64_t> samples, segments;     // [S]: since the stream's last reset
    std::vector<uint32_t> carry_n, flip;         // [S]: the carry's length, and which of the two buffers holds it
    uint64_t pushed_calls = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;       // set by the measurement hook only: recorded around the launches of a push
};
// (the stride the kernel was written against, tone_search.h: kToneSearchGuard / 2 doubles, or samples, on either side)
static_assert(Guarded<double>::stride_of(hd::kToneSearchSeg, hd::kToneSearchGuard) == hd::kToneSearchSeg + hd::kToneSearchGuard, "tone search accumulator stride");
static_assert(Guarded<float2>::stride_of(hd::kToneSearchSeg, hd::kToneSearchGuard) == hd::kToneSearchSeg + hd::kToneSearchGuard, "tone search carry stride");

namespace {

// Its own per chunk: the stream's carry, the segments the chunk completes and which carry buffer is read go into the descriptor, and the streams' counts
// move on behind every launch's wait.  (The kernel's LDS is static: its launch always fits.)
int tone_search_launch(hd_tone_search* ts, uint32_t max_n)
{
    if (const int rc = check_max_push(ts, "hd_tone_search", &max_n, [](uint32_t) {})) return rc;
    return launch_chunks(
        ts, max_n, HD_TONE_SEARCH_CHUNK, "",
        [&](uint32_t s, hd::ToneSearchSrc& d) {
            d.carry = ts->carry_n[s];
            d.segs = hd::tone_search_segments(d.carry, d.n);
            d.flip = ts->flip[s];
        },
        [&] {
            hd::launch_tone_search(ts->e->qa, ts->S, ts->src.dev, ts->win.p, ts->tw, ts->acc.base(), ts->acc.stride, ts->carry.base(), ts->carry.stride);
            return true;
        },
        [&] {
            for (uint32_t s = 0; s < ts->S; ++s) {
                const hd::ToneSearchSrc& d = ts->src.p[s];
                ts->samples[s] += d.n;
                ts->segments[s] += d.segs;
                ts->carry_n[s] = d.carry + d.n - d.segs * hd::kToneSearchStep;
                if (d.segs) ts->flip[s] ^= 1u;
            }
        });
}

// (The carry buffers need no clearing: nothing behind a stream's carry length is read.)
int tone_search_clear(hd_tone_search* ts, uint32_t s0, uint32_t ns)
{
    hipStream_t q = ts->e->qa;
    HD_HIP(hipMemset2DAsync(ts->acc.row(s0), ts->acc.stride * sizeof(double), 0,
                            (size_t)hd::kToneSearchSeg * sizeof(double), ns, q));
    HD_HIP(hipStreamSynchronize(q));
    for (uint32_t s = s0; s < s0 + ns; ++s) { ts->samples[s] = ts->segments[s] = 0; ts->carry_n[s] = ts->flip[s] = 0; }
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_tone_search_params_default(hd_tone_search_params* p) { if (p) *p = hd_tone_search_params{0u, 0u}; }
void hd_tone_search_detect_params_default(hd_tone_search_detect_params* p) { if (p) hd::tone_search_detect_params_default(p); }

int hd_tone_search_create(hd_engine* e, const hd_tone_search_params* params, hd_tone_search** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_tone_search> ts(new hd_tone_search);
    ts->e = e; ts->S = e->S;
    if (params) ts->prm = *params;
    if (const int rc = default_max_push(e, &ts->prm.max_push, "tone search")) return rc;
    if (const int rc = enter(e)) return rc;
    const uint32_t S = ts->S;
    ts->samples.assign(S, 0); ts->segments.assign(S, 0); ts->carry_n.assign(S, 0u); ts->flip.assign(S, 0u);
    std::vector<float> w(hd::kToneSearchSeg);
    hd::survey_window(w.data());
    for (float v : w) ts->sum_w2 += (double)v * (double)v;
    std::vector<float2> tw_host;
    HD_HIP(ts->acc.alloc(S, hd::kToneSearchSeg, hd::kToneSearchGuard, hd::kToneSearchGuardWord, e->qa));
    HD_HIP(ts->carry.alloc((size_t)S * 2, hd::kToneSearchSeg, hd::kToneSearchGuard, hd::kToneSearchGuardWord, e->qa));
    HD_HIP(ts->win.alloc_unfilled(w.size()));
    HD_HIP(ts->src.alloc(S));
    if (const int rc = hd::eng::engine_or_own_twiddles(e, ts->own_tw, tw_host, e->qa, &ts->tw)) return rc;
    HD_HIP(hipMemcpyAsync(ts->win.p, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, e->qa));
    if (const int rc = tone_search_clear(ts.get(), 0, S)) return rc;   // (waits for the queue: the tables are locals)
    *out = ts.release();
    return HD_OK;
}

void hd_tone_search_destroy(hd_tone_search* ts) { destroy(ts); }

int hd_tone_search_reset(hd_tone_search* ts, uint32_t stream) { return reset(ts, stream, tone_search_clear); }

int hd_tone_search_push_engine(hd_tone_search* ts) { return push_engine(ts, "hd_tone_search_push_engine", tone_search_launch); }

int hd_tone_search_push_device(hd_tone_search* ts, const float* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(ts, reinterpret_cast<const float2*>(d_iq), stride, n_per_stream, n, true, tone_search_launch);
}

int hd_tone_search_push_host(hd_tone_search* ts, const float* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(ts, reinterpret_cast<const float2*>(iq), stride, n_per_stream, n, false, tone_search_launch);
}

int hd_tone_search_power(hd_tone_search* ts, uint32_t stream, double* p, size_t cap, uint64_t* segments)
{
    if (const int rc = check_object(ts, stream)) return rc;
    if (!p) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(ts->e->mtx);
    if (const int rc = enter(ts->e)) return rc;
    const uint64_t segs = ts->segments[stream];
    if (segments) *segments = segs;
    if (cap < hd::kToneSearchSeg) return 0;
    // (no queue to wait for: every push has waited for its launches)
    HD_HIP(hipMemcpy(p, ts->acc.row(stream), hd::kToneSearchSeg * sizeof(double), hipMemcpyDeviceToHost));
    const double norm = (double)segs * ts->sum_w2;
    for (uint32_t i = 0; i < hd::kToneSearchSeg; ++i) p[i] = segs ? p[i] / norm : 0.0;
    return (int)hd::kToneSearchSeg;
}

int hd_tone_search_stats(hd_tone_search* ts, uint32_t stream, hd_tone_search_info* out)
{
    if (const int rc = check_object(ts, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(ts->e->mtx);
    *out = hd_tone_search_info{ts->samples[stream], ts->segments[stream], ts->carry_n[stream], 0u};
    return HD_OK;
}

int hd_tone_search_detect(hd_tone_search* ts, uint32_t stream, const hd_tone_search_detect_params* p, hd_tone_search_result* out)
{
    if (const int rc = check_object(ts, stream)) return rc;
    if (!p || !out) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(ts->e->mtx);
    std::vector<double> pw(hd::kToneSearchSeg);
    uint64_t segs = 0;
    const int n = hd_tone_search_power(ts, stream, pw.data(), pw.size(), &segs);
    if (n < 0) return n;
    const int rc = hd::tone_search_detect(pw.data(), segs, ts->e->fsd, p, out);
    if (rc == HD_ERR_UNSUPPORTED) return fail(rc, "hd_tone_search_detect needs at least 8 segments (" + std::to_string(segs) + " so far)");
    if (rc) return fail(rc, "hd_tone_search_detect: baud > 0, 0 < shift_lo_hz <= shift_hi_hz, and a tone spacing that fits the spectrum");
    return HD_OK;
}

int hd_debug_tone_search_push_timed(hd_tone_search* ts, float* kernel_ms, double* host_us) { return push_timed(ts, kernel_ms, host_us, hd_tone_search_push_engine); }

// Test hook (tests/test_gpu_tone_search.py; not part of the ABI): how many of the guard words around the stream's accumulator and its two carry buffers no
// longer hold their pattern.
int hd_debug_tone_search_guards(hd_tone_search* ts, uint32_t stream)
{
    if (!ts || stream >= ts->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(ts->e->mtx);
    if (const int rc = enter(ts->e)) return rc;
    return damaged_guards({{ts->acc, stream}, {ts->carry, (size_t)stream * 2}, {ts->carry, (size_t)stream * 2 + 1}});
}

}  // extern "C"

/* ---------------------------------------------------------------- diversity combiner (kernels/combine.hip) ----------------------------- */

struct hd_combine {
    static constexpr const char* kNull = "null combiner";
    hd_engine* e = nullptr;
    hd_combine_params prm{};
    uint32_t S = 0;
    Guarded<int16_t> ring;                       // [S]: guard | HD_COMBINE_RING samples | guard
    Guarded<float> rows;                         // [S]: guard | max_push floats | guard
    DevBuf<int32_t> scores;                      // [7][2 * HD_COMBINE_MAX_LAG + 1]: the last search's, allocated by the first search
    DevBuf<float> slab;                          // hd_combine_push_host: the rows packed end to end, grown on demand
    PinBuf<hd::CombineSrc> src;                  // [S]: a launch's descriptors, read by the kernel in place (a launch is waited for before the next is written)
    PinBuf<hd::CombineGroup> grp;                // [S]: a push's groups, in the order of `refs`
    PinBuf<hd_combine_lag> res;                  // [7]: the last search's results, written by the kernel in place
    std::vector<uint32_t> group_of, delay, weight, row_n;       // [S]: the stream's reference (HD_COMBINE_NO_GROUP: in no group), its delay and weight, its row's length
    std::vector<std::vector<uint32_t>> members;  // [S]: by reference, the group's streams, the reference first
    std::vector<uint64_t> count;                 // [S]: by reference, the group's samples since its last reset
    std::vector<uint32_t> refs;                  // the references, ascending
    std::vector<uint32_t> searched;              // the members of the last search, the reference first
    uint32_t searched_L = 0;
    uint64_t pushed_calls = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;       // set by the measurement hook only: recorded around the launches of a push
};
// (the strides the kernel was written against, combine.h: 2 kCombineGuard int16 samples on either side of the ring)
static_assert(Guarded<int16_t>::stride_of(HD_COMBINE_RING, hd::kCombineGuard) == HD_COMBINE_RING + 4 * hd::kCombineGuard, "combiner ring stride");
static_assert(Guarded<float>::stride_of(4096, hd::kCombineGuard) == 4096 + 2 * hd::kCombineGuard, "combiner row stride");

namespace {

void combine_list_refs(hd_combine* c)
{
    c->refs.clear();
    for (uint32_t s = 0; s < c->S; ++s) if (c->group_of[s] == s) c->refs.push_back(s);
}

// Stream s leaves its group; a group that loses its reference is dissolved.
void combine_leave(hd_combine* c, uint32_t s)
{
    const uint32_t r = c->group_of[s];
    if (r == HD_COMBINE_NO_GROUP) return;
    auto& mem = c->members[r];
    if (r == s) {
        for (uint32_t m : mem) { c->group_of[m] = HD_COMBINE_NO_GROUP; c->row_n[m] = 0; }
        mem.clear();
        c->count[r] = 0;
    } else {
        mem.erase(std::find(mem.begin(), mem.end(), s));
        c->group_of[s] = HD_COMBINE_NO_GROUP;
    }
}

hd::CombineGroup combine_group(const hd_combine* c, uint32_t r)
{
    hd::CombineGroup g{};
    const auto& mem = c->members[r];
    g.base = c->count[r];
    g.count = (uint32_t)mem.size();
    for (uint32_t m = 0; m < g.count; ++m) { g.stream[m] = mem[m]; g.delay[m] = c->delay[mem[m]]; g.weight[m] = c->weight[mem[m]]; g.wt += g.weight[m]; }
    g.wt = std::max(g.wt, 1u);
    return g;
}

// Its own: a stream in no group is passed by and the members of a group must bring the same length, both in front of the max_push test; the groups'
// descriptors hold for every chunk of the push (a sample's absolute index is base + off + j); the groups' counts move on behind the last chunk.
int combine_launch(hd_combine* c, uint32_t max_n)
{
    for (uint32_t s = 0; s < c->S; ++s) if (c->group_of[s] == HD_COMBINE_NO_GROUP) c->src.p[s].n_total = 0;
    for (uint32_t r : c->refs)
        for (uint32_t m : c->members[r])
            if (c->src.p[m].n_total != c->src.p[r].n_total)
                return fail(HD_ERR_INVALID, "hd_combine: stream " + std::to_string(m) + " brings " + std::to_string(c->src.p[m].n_total) + " samples, its group's reference " +
                                                std::to_string(r) + " brings " + std::to_string(c->src.p[r].n_total));
    if (const int rc = check_max_push(c, "hd_combine", &max_n, [](uint32_t) {})) return rc;
    for (uint32_t s = 0; s < c->S; ++s) c->row_n[s] = c->group_of[s] == s ? c->src.p[s].n_total : 0u;
    const uint32_t ng = (uint32_t)c->refs.size();
    for (uint32_t k = 0; k < ng; ++k) c->grp.p[k] = combine_group(c, c->refs[k]);
    uint32_t cap = 0;
    const int rc = launch_chunks(
        c, max_n, HD_COMBINE_CHUNK, "",
        [&](uint32_t, const hd::CombineSrc& d) { cap = std::max(cap, d.n); },
        [&] {
            hd::launch_combine(c->e->qa, ng, cap, c->src.dev, c->grp.dev, c->ring.base(), c->ring.stride, c->rows.base(), c->rows.stride, c->prm.max_push);
            cap = 0;
            return true;
        },
        [] {});
    if (rc) return rc;
    for (uint32_t r : c->refs) c->count[r] += c->src.p[r].n_total;
    return HD_OK;
}

// (The rings need no clearing: nothing in front of a group's index 0 is read.)  One stream: it must be a reference.
int combine_clear(hd_combine* c, uint32_t s0, uint32_t ns)
{
    if (ns == 1 && c->group_of[s0] != s0) return fail(HD_ERR_INVALID, "hd_combine_reset: stream " + std::to_string(s0) + " is no group's reference");
    for (uint32_t s = s0; s < s0 + ns; ++s) {
        if (c->group_of[s] != s) continue;
        c->count[s] = 0;
        for (uint32_t m : c->members[s]) c->row_n[m] = 0;
    }
    return HD_OK;
}

// hd_combine_lags behind the lock and enter(): the search's two kernels on the engine's first queue and the wait for them.
int combine_search(hd_combine* c, uint32_t ref, const hd_combine_lag_params* p, hd_combine_lag* out, size_t cap)
{
    if (c->group_of[ref] != ref) return fail(HD_ERR_INVALID, "hd_combine_lags: stream " + std::to_string(ref) + " is no group's reference");
    if (!hd::combine_lag_params_ok(p))
        return fail(HD_ERR_INVALID, "hd_combine_lags: window a multiple of 64 in 1024 .. 16384, max_lag a multiple of 64 in 64 .. 4096, guard >= 1");
    const hd::CombineGroup g = combine_group(c, ref);
    if (cap < g.count) return fail(HD_ERR_INVALID, "hd_combine_lags: room for " + std::to_string(cap) + " results, the group has " + std::to_string(g.count) + " members");
    const uint64_t n = c->count[ref], need = (uint64_t)p->window + 2u * (uint64_t)p->max_lag;
    if (n < need) return fail(HD_ERR_UNSUPPORTED, "hd_combine_lags needs " + std::to_string(need) + " samples (" + std::to_string(n) + " so far)");
    if (!c->scores.p) HD_HIP(c->scores.alloc_unfilled((size_t)(HD_COMBINE_MAX_MEMBERS - 1) * (2 * HD_COMBINE_MAX_LAG + 1)));
    hd::launch_combine_lags(c->e->qa, &g, n, p->window, p->max_lag, p->guard, p->min_peak_q8, p->min_margin_q8, c->ring.base(), c->ring.stride, c->scores.p, c->res.dev);
    HD_HIP(hipGetLastError());
    HD_HIP(hipStreamSynchronize(c->e->qa));
    std::atomic_thread_fence(std::memory_order_acquire);
    out[0] = hd_combine_lag{ref, 0, (int32_t)p->window, 0, 1u};
    for (uint32_t m = 1; m < g.count; ++m) out[m] = c->res.p[m - 1];
    c->searched.assign(g.stream, g.stream + g.count);
    c->searched_L = p->max_lag;
    return HD_OK;
}

// (the engine's mutex is held)
int combine_member(hd_combine* c, uint32_t stream, const char* fn)
{
    if (c->group_of[stream] == HD_COMBINE_NO_GROUP) return fail(HD_ERR_INVALID, std::string(fn) + ": stream " + std::to_string(stream) + " is in no group");
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_combine_params_default(hd_combine_params* p) { if (p) *p = hd_combine_params{0u, 0u}; }
void hd_combine_lag_params_default(hd_combine_lag_params* p) { if (p) hd::combine_lag_params_default(p); }

int hd_combine_create(hd_engine* e, const hd_combine_params* params, hd_combine** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_combine> c(new hd_combine);
    c->e = e; c->S = e->S;
    if (params) c->prm = *params;
    if (const int rc = default_max_push(e, &c->prm.max_push, "combiner")) return rc;
    if (const int rc = enter(e)) return rc;
    const uint32_t S = c->S;
    c->group_of.assign(S, HD_COMBINE_NO_GROUP); c->delay.assign(S, 0u); c->weight.assign(S, 256u); c->row_n.assign(S, 0u);
    c->members.assign(S, {}); c->count.assign(S, 0);
    HD_HIP(c->ring.alloc(S, HD_COMBINE_RING, hd::kCombineGuard, hd::kCombineGuardWord, e->qa));
    HD_HIP(c->rows.alloc(S, c->prm.max_push, hd::kCombineGuard, hd::kCombineGuardWord, e->qa));
    HD_HIP(c->src.alloc(S));
    HD_HIP(c->grp.alloc(S));
    HD_HIP(c->res.alloc(HD_COMBINE_MAX_MEMBERS - 1));
    HD_HIP(hipStreamSynchronize(e->qa));
    *out = c.release();
    return HD_OK;
}

void hd_combine_destroy(hd_combine* c) { destroy(c); }

int hd_combine_reset(hd_combine* c, uint32_t ref) { return reset(c, ref, combine_clear); }

int hd_combine_set_group(hd_combine* c, const uint32_t* streams, uint32_t count)
{
    if (!c) return fail(HD_ERR_INVALID, hd_combine::kNull);
    if (!streams) return fail(HD_ERR_INVALID, "null streams");
    if (count > HD_COMBINE_MAX_MEMBERS) return fail(HD_ERR_INVALID, "hd_combine_set_group: at most " + std::to_string(HD_COMBINE_MAX_MEMBERS) + " members");
    for (uint32_t a = 0; a < std::max(count, 1u); ++a) {
        if (streams[a] >= c->S) return fail(HD_ERR_INVALID, "stream index out of range");
        for (uint32_t b = 0; b < a; ++b) if (streams[a] == streams[b]) return fail(HD_ERR_INVALID, "hd_combine_set_group: stream " + std::to_string(streams[a]) + " is named twice");
    }
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (!count) {
        if (c->group_of[streams[0]] != streams[0]) return fail(HD_ERR_INVALID, "hd_combine_set_group: stream " + std::to_string(streams[0]) + " is no group's reference");
        combine_leave(c, streams[0]);
        combine_list_refs(c);
        return HD_OK;
    }
    for (uint32_t a = 0; a < count; ++a) combine_leave(c, streams[a]);
    const uint32_t r = streams[0];
    c->members[r].assign(streams, streams + count);
    c->count[r] = 0;
    for (uint32_t a = 0; a < count; ++a) { const uint32_t s = streams[a]; c->group_of[s] = r; c->delay[s] = 0; c->weight[s] = 256; c->row_n[s] = 0; }
    combine_list_refs(c);
    return HD_OK;
}

int hd_combine_set_delay(hd_combine* c, uint32_t stream, uint32_t delay)
{
    if (const int rc = check_object(c, stream)) return rc;
    if (delay > HD_COMBINE_MAX_DELAY) return fail(HD_ERR_INVALID, "hd_combine_set_delay: at most " + std::to_string(HD_COMBINE_MAX_DELAY) + " samples");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = combine_member(c, stream, "hd_combine_set_delay")) return rc;
    c->delay[stream] = delay;
    return HD_OK;
}

int hd_combine_set_weight(hd_combine* c, uint32_t stream, uint32_t weight)
{
    if (const int rc = check_object(c, stream)) return rc;
    if (weight > 256u) return fail(HD_ERR_INVALID, "hd_combine_set_weight: at most 256");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = combine_member(c, stream, "hd_combine_set_weight")) return rc;
    c->weight[stream] = weight;
    return HD_OK;
}

int hd_combine_push_engine(hd_combine* c) { return push_engine(c, "hd_combine_push_engine", combine_launch); }

int hd_combine_push_device(hd_combine* c, const float* d_rows, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(c, d_rows, stride, n_per_stream, n, true, combine_launch);
}

int hd_combine_push_host(hd_combine* c, const float* rows, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(c, rows, stride, n_per_stream, n, false, combine_launch);
}

int hd_combine_rows(hd_combine* c, const float** d_rows, size_t* stride, uint32_t* n_per_stream) { return output_rows(c, d_rows, stride, n_per_stream); }

int hd_combine_output(hd_combine* c, uint32_t stream, float* out, size_t cap) { return output_row(c, stream, out, cap); }

int hd_combine_stats(hd_combine* c, uint32_t stream, hd_combine_info* out)
{
    if (const int rc = check_object(c, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    const uint32_t r = c->group_of[stream];
    if (r == HD_COMBINE_NO_GROUP) *out = hd_combine_info{0u, HD_COMBINE_NO_GROUP, 0u, 0u, 0u};
    else *out = hd_combine_info{c->count[r], r, c->delay[stream], c->weight[stream], (uint32_t)c->members[r].size()};
    return HD_OK;
}

int hd_combine_lags(hd_combine* c, uint32_t ref, const hd_combine_lag_params* p, hd_combine_lag* out, size_t cap)
{
    if (const int rc = check_object(c, ref)) return rc;
    if (!p || !out) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = enter(c->e)) return rc;
    return combine_search(c, ref, p, out, cap);
}

int hd_combine_align(hd_combine* c, uint32_t ref, const hd_combine_lag_params* p, hd_combine_lag* out, size_t cap)
{
    if (const int rc = check_object(c, ref)) return rc;
    if (!p || !out) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = enter(c->e)) return rc;
    if (const int rc = combine_search(c, ref, p, out, cap)) return rc;
    const auto& mem = c->members[ref];
    uint32_t d[HD_COMBINE_MAX_MEMBERS], w[HD_COMBINE_MAX_MEMBERS];
    for (size_t m = 0; m < mem.size(); ++m) { d[m] = c->delay[mem[m]]; w[m] = c->weight[mem[m]]; }
    const int valid = hd::combine_align(out, (uint32_t)mem.size(), d, w);
    for (size_t m = 0; m < mem.size(); ++m) { c->delay[mem[m]] = d[m]; c->weight[mem[m]] = w[m]; }
    return valid;
}

// The measurement hook (tools/micro/combine_rate.py; not part of the ABI): hd_combine_push_device of the rows, its kernels between two HIP events.
int hd_debug_combine_push_timed(hd_combine* c, const float* d_rows, size_t stride, const uint32_t* n_per_stream, uint32_t n, float* kernel_ms, double* host_us)
{
    if (!c) return fail(HD_ERR_INVALID, hd_combine::kNull);
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    const uint64_t keep = c->pushed_calls;                           // (push_timed reads the events where the push moved this count: moved here, put back below)
    const int rc = push_timed(c, kernel_ms, host_us, [&](hd_combine* o) {
        const int r = hd_combine_push_device(o, d_rows, stride, n_per_stream, n);
        if (r == HD_OK) o->pushed_calls = keep + 1;
        return r;
    });
    c->pushed_calls = keep;
    return rc;
}

// Test hook (tests/test_gpu_combine.py; not part of the ABI): the 2 L + 1 scores of `stream` in the last search; returns their number, 0 where the stream
// was no member of it beside the reference; nothing is written where cap is below it.
int hd_debug_combine_scores(hd_combine* c, uint32_t stream, int32_t* out, size_t cap)
{
    if (!c || stream >= c->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = enter(c->e)) return rc;
    const size_t k = 2 * (size_t)c->searched_L + 1;
    for (size_t m = 1; m < c->searched.size(); ++m) {
        if (c->searched[m] != stream) continue;
        if (out && cap >= k) HD_HIP(hipMemcpy(out, c->scores.p + (m - 1) * k, k * sizeof(int32_t), hipMemcpyDeviceToHost));
        return (int)k;
    }
    return 0;
}

// Test hook (tests/test_gpu_combine.py; not part of the ABI): how many of the guard words around the stream's ring and its row no longer hold their pattern.
int hd_debug_combine_guards(hd_combine* c, uint32_t stream)
{
    if (!c || stream >= c->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(c->e->mtx);
    if (const int rc = enter(c->e)) return rc;
    return damaged_guards({{c->ring, stream}, {c->rows, stream}});
}

}  // extern "C"

/* ---------------------------------------------------------------- SSDV packets (kernels/ssdv.hip) -------------------------------------- */

struct hd_ssdv {
    static constexpr const char* kNull = "null SSDV object";
    static constexpr uint32_t kStage = 1u << 18;  // words of one scan round's upload
    hd_engine* e = nullptr;
    hd_ssdv_params prm{};
    uint32_t S = 0;
    Guarded<uint32_t> ring;                      // [S]: guard | HD_SSDV_RING words | guard
    Guarded<uint32_t> cnt;                       // one row: guard | the launch's accepted candidates, [S] crc_bad | guard
    Guarded<uint32_t> out;                       // one row: guard | HD_SSDV_LAUNCH results (hd::SsdvOut) | guard
    DevBuf<hd::SsdvTables> tab;
    PinBuf<hd::SsdvSrc> src;                     // [S]: a launch's descriptors, read by the kernels in place (a launch is waited for before the next is written)
    PinBuf<uint32_t> stage;                      // [kStage]: a round's new words, stream behind stream, read by k_ssdv_append in place
    std::vector<hd::SsdvStream> st;              // [S]: the doors, the delivery and the counters; `words` holds what is not uploaded yet
    std::vector<uint64_t> up;                    // [S]: words uploaded since the stream's last reset
    std::vector<uint32_t> h_cnt;
    std::vector<hd::SsdvOut> h_out, found;       // a launch's results; a scan's
    bool launched = false;                       // the last scan launched k_ssdv_scan (the measurement hook's question)
    hipEvent_t t0 = nullptr, t1 = nullptr;       // set by the measurement hook only: recorded around the launches of a scan's last round
};
// (the stride the kernels were written against, ssdv.h)
static_assert(Guarded<uint32_t>::stride_of(HD_SSDV_RING, hd::kSsdvGuard) == HD_SSDV_RING + 2 * hd::kSsdvGuard, "SSDV ring stride");

namespace {

constexpr size_t kSsdvOutWords = sizeof(hd::SsdvOut) / sizeof(uint32_t);

// One round: up to HD_SSDV_RING - 256 new words per stream go up (a ring then holds every word of every candidate the round decides, and the append
// writes no slot a candidate of an earlier round still needs: those are decided), then every position that is decided now is launched, at most
// HD_SSDV_LAUNCH candidates over all streams per launch, so that the results of a launch always fit.  Rounds until nothing is left; then the results
// are sorted by (stream, pos) and delivered -- which packets a scan delivers cannot depend on the order in which waves finished.
int ssdv_scan(hd_ssdv* v)
{
    hipStream_t q = v->e->qa;
    v->found.clear();
    v->launched = false;
    for (;;) {
        uint32_t used = 0, max_new = 0, max_cand = 0, active = 0;
        for (uint32_t s = 0; s < v->S; ++s) {
            hd::SsdvStream& st = v->st[s];
            hd::SsdvSrc& d = v->src.p[s];
            const uint32_t take = (uint32_t)std::min<uint64_t>({st.n - v->up[s], (uint64_t)HD_SSDV_RING - 256u, (uint64_t)hd_ssdv::kStage - used});
            if (take) std::memcpy(v->stage.p + used, st.words.data() + (size_t)(v->up[s] - st.first), (size_t)take * sizeof(uint32_t));
            d.append_pos = v->up[s]; d.stage_at = used; d.stage_n = take;
            used += take; v->up[s] += take;
            st.drop(v->up[s]);
            d.base = st.decided;
            d.n_total = v->up[s] >= 256u ? (uint32_t)(v->up[s] - 255u - st.decided) : 0u;
            d.off = 0; d.n = 0;
            max_new = std::max(max_new, take); max_cand = std::max(max_cand, d.n_total);
            active += d.n_total != 0;
        }
        if (!max_new && !max_cand) break;
        std::atomic_thread_fence(std::memory_order_release);
        hd::launch_ssdv_append(q, v->S, max_new, v->src.dev, v->stage.dev, v->ring.base(), v->ring.stride);
        HD_HIP(hipGetLastError());
        if (!max_cand) { HD_HIP(hipStreamSynchronize(q)); continue; }
        uint32_t cap = 0;
        hipError_t fetch = hipSuccess;
        const int rc = launch_chunks(
            v, max_cand, std::max(1u, (uint32_t)HD_SSDV_LAUNCH / active), "",
            [&](uint32_t, const hd::SsdvSrc& d) { cap = std::max(cap, d.n); },
            [&] {
                if (hipMemsetAsync(v->cnt.row(0), 0, (size_t)(1 + v->S) * sizeof(uint32_t), q) != hipSuccess) return false;
                hd::launch_ssdv_scan(q, v->S, cap, v->src.dev, v->tab.p, v->ring.base(), v->ring.stride, v->cnt.row(0),
                                     reinterpret_cast<hd::SsdvOut*>(v->out.row(0)), HD_SSDV_LAUNCH);
                cap = 0;
                return true;
            },
            [&] {                                // the launch is done: its counters, and its results if it has any
                if (fetch != hipSuccess) return;
                fetch = hipMemcpy(v->h_cnt.data(), v->cnt.row(0), v->h_cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
                if (fetch != hipSuccess) return;
                for (uint32_t s = 0; s < v->S; ++s) v->st[s].crc_bad += v->h_cnt[1 + s];
                const size_t k = std::min<size_t>(v->h_cnt[0], HD_SSDV_LAUNCH);
                if (!k) return;
                fetch = hipMemcpy(v->h_out.data(), v->out.row(0), k * sizeof(hd::SsdvOut), hipMemcpyDeviceToHost);
                if (fetch == hipSuccess) v->found.insert(v->found.end(), v->h_out.begin(), v->h_out.begin() + k);
            });
        if (rc) return rc;
        HD_HIP(fetch);
        v->launched = true;
        for (uint32_t s = 0; s < v->S; ++s) v->st[s].decided += v->src.p[s].n_total;
    }
    std::sort(v->found.begin(), v->found.end(), [](const hd::SsdvOut& a, const hd::SsdvOut& b) { return a.stream != b.stream ? a.stream < b.stream : a.pos < b.pos; });
    for (const hd::SsdvOut& r : v->found) {
        if (r.stream >= v->S) continue;
        hd_ssdv_packet p;
        std::memset(&p, 0, sizeof p);
        p.pos = r.pos; p.trial = r.trial; p.errors = r.errors; p.erasures = r.erasures; p.erasures_changed = r.changed;
        std::memcpy(p.data, r.data, sizeof p.data);
        hd::ssdv_header(&p);
        v->st[r.stream].deliver(p);
    }
    return HD_OK;
}

int ssdv_clear(hd_ssdv* v, uint32_t s0, uint32_t ns)
{
    for (uint32_t s = s0; s < s0 + ns; ++s) { v->st[s].reset(); v->up[s] = 0; }
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_ssdv_params_default(hd_ssdv_params* p) { if (p) hd::ssdv_params_default(p); }

int hd_ssdv_create(hd_engine* e, const hd_ssdv_params* params, hd_ssdv** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_ssdv> v(new hd_ssdv);
    v->e = e; v->S = e->S;
    hd::ssdv_params_default(&v->prm);
    if (params) v->prm = *params;
    if (!hd::ssdv_params_ok(&v->prm)) return fail(HD_ERR_INVALID, "SSDV parameters: max_fill <= 64");
    // (a launch takes at least one candidate of every active stream and its results must fit HD_SSDV_LAUNCH slots)
    if (e->S > HD_SSDV_LAUNCH) return fail(HD_ERR_UNSUPPORTED, "hd_ssdv_create: at most " + std::to_string(HD_SSDV_LAUNCH) + " streams");
    if (const int rc = enter(e)) return rc;
    const uint32_t S = v->S;
    v->st.resize(S); v->up.assign(S, 0);
    for (auto& st : v->st) st.max_fill = v->prm.max_fill;
    v->h_cnt.assign(1 + (size_t)S, 0u); v->h_out.resize(HD_SSDV_LAUNCH);
    HD_HIP(v->ring.alloc(S, HD_SSDV_RING, hd::kSsdvGuard, hd::kSsdvGuardWord, e->qa));
    HD_HIP(v->cnt.alloc(1, 1 + (size_t)S, hd::kSsdvGuard, hd::kSsdvGuardWord, e->qa));
    HD_HIP(v->out.alloc(1, (size_t)HD_SSDV_LAUNCH * kSsdvOutWords, hd::kSsdvGuard, hd::kSsdvGuardWord, e->qa));
    HD_HIP(v->tab.alloc_unfilled(1));
    HD_HIP(v->src.alloc(S));
    HD_HIP(v->stage.alloc(hd_ssdv::kStage));
    std::unique_ptr<hd::SsdvTables> t(new hd::SsdvTables);
    const hd::SsdvField& F = hd::ssdv_field();
    for (uint32_t l = 0; l < 64; ++l) {
        uint8_t pw[4] = {1, 1, 1, 1};
        for (uint32_t k = 0; k <= 32; ++k) {
            t->chien[k][l] = (uint32_t)pw[0] | (uint32_t)pw[1] << 8 | (uint32_t)pw[2] << 16 | (uint32_t)pw[3] << 24;
            for (uint32_t b = 0; b < 4; ++b) pw[b] = F.mul(pw[b], F.loc[255u - (l + 64u * b)]);
        }
    }
    std::memcpy(t->loc, F.loc, sizeof t->loc);
    for (uint32_t m = 0; m < 32; ++m) {
        for (uint32_t k = 0; k < 8; ++k) t->rootmul[m][k] = F.mul(F.root[m], F.exp[k]);
        t->root127[m] = F.exp[((uint32_t)F.log[F.root[m]] * 127u) % 255u];
    }
    HD_HIP(hipMemcpyAsync(v->tab.p, t.get(), sizeof(hd::SsdvTables), hipMemcpyHostToDevice, e->qa));
    HD_HIP(hipStreamSynchronize(e->qa));         // (`t` is a local)
    *out = v.release();
    return HD_OK;
}

void hd_ssdv_destroy(hd_ssdv* v) { destroy(v); }

int hd_ssdv_reset(hd_ssdv* v, uint32_t stream) { return reset(v, stream, ssdv_clear); }

int hd_ssdv_push_bytes(hd_ssdv* v, uint32_t stream, const uint8_t* bytes, const uint32_t* conf, size_t n)
{
    if (const int rc = check_object(v, stream)) return rc;
    if (n && !bytes) return fail(HD_ERR_INVALID, "null bytes");
    std::lock_guard<std::recursive_mutex> lock(v->e->mtx);
    if (const int rc = enter(v->e)) return rc;
    v->st[stream].push_bytes(bytes, conf, n);
    return HD_OK;
}

int hd_ssdv_push_records(hd_ssdv* v, uint32_t stream, const hd_clocked_record* records, size_t n, uint32_t char_len)
{
    if (const int rc = check_object(v, stream)) return rc;
    if (n && !records) return fail(HD_ERR_INVALID, "null records");
    std::lock_guard<std::recursive_mutex> lock(v->e->mtx);
    if (const int rc = enter(v->e)) return rc;
    v->st[stream].push_records(records, n, char_len);
    return HD_OK;
}

int hd_ssdv_scan(hd_ssdv* v)
{
    if (!v) return fail(HD_ERR_INVALID, hd_ssdv::kNull);
    std::lock_guard<std::recursive_mutex> lock(v->e->mtx);
    if (const int rc = enter(v->e)) return rc;
    return ssdv_scan(v);
}

int hd_ssdv_push_clocked(hd_ssdv* v, hd_clocked* c)
{
    if (!v) return fail(HD_ERR_INVALID, hd_ssdv::kNull);
    if (!c) return fail(HD_ERR_INVALID, hd_clocked::kNull);
    if (v->e != c->e) return fail(HD_ERR_INVALID, "hd_ssdv_push_clocked: the two objects belong to different engines");
    std::lock_guard<std::recursive_mutex> lock(v->e->mtx);
    if (const int rc = enter(v->e)) return rc;
    std::vector<hd::ClockedState> hs(c->S);      // one copy says which streams have records waiting
    HD_HIP(hipMemcpy(hs.data(), c->st.p, hs.size() * sizeof(hd::ClockedState), hipMemcpyDeviceToHost));
    std::vector<hd_clocked_record> buf;
    for (uint32_t s = 0; s < v->S; ++s) {
        const hd::ClockedState& m = c->modem[s];
        if (!m.F || m.nbits != 8u || hs[s].written == hs[s].taken) continue;
        buf.resize((size_t)(hs[s].written - hs[s].taken));
        size_t n = 0;
        if (const int rc = clocked_drain(c, s, buf.data(), buf.size(), &n)) return rc;
        const uint32_t char_len = (uint32_t)(((uint64_t)(1u + m.nbits + m.nstops) * m.F + 32768u) >> 16);
        v->st[s].push_records(buf.data(), n, char_len);
    }
    return ssdv_scan(v);
}

int hd_ssdv_take_packets(hd_ssdv* v, uint32_t stream, hd_ssdv_packet* out, size_t cap)
{
    if (const int rc = check_object(v, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(v->e->mtx);
    if (const int rc = enter(v->e)) return rc;
    return (int)v->st[stream].take(out, cap);
}

int hd_ssdv_stats(hd_ssdv* v, uint32_t stream, hd_ssdv_counters* out)
{
    if (const int rc = check_object(v, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(v->e->mtx);
    if (const int rc = enter(v->e)) return rc;
    v->st[stream].stats(out);
    return HD_OK;
}

// The measurement hook (tools/micro/ssdv_rate.py; not part of the ABI): hd_ssdv_push_clocked (c null: hd_ssdv_scan), the host time of the whole call
// in microseconds and the launches of its last round between two HIP events (0 where k_ssdv_scan was not launched).
int hd_debug_ssdv_scan_timed(hd_ssdv* v, hd_clocked* c, float* kernel_ms, double* host_us)
{
    if (!v || !kernel_ms || !host_us) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(v->e->mtx);
    if (const int rc = enter(v->e)) return rc;
    HD_HIP(hipEventCreate(&v->t0));
    HD_HIP(hipEventCreate(&v->t1));
    const auto w0 = std::chrono::steady_clock::now();
    const int rc = c ? hd_ssdv_push_clocked(v, c) : hd_ssdv_scan(v);
    *host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
    *kernel_ms = 0;
    if (rc == HD_OK && v->launched && hipEventQuery(v->t1) == hipSuccess) (void)hipEventElapsedTime(kernel_ms, v->t0, v->t1);
    (void)hipGetLastError();
    (void)hipEventDestroy(v->t0); (void)hipEventDestroy(v->t1);
    v->t0 = v->t1 = nullptr;
    return rc;
}

// Test hook (tests/test_gpu_ssdv.py; not part of the ABI): how many of the guard words around the stream's ring, the counters and the results no longer
// hold their pattern.
int hd_debug_ssdv_guards(hd_ssdv* v, uint32_t stream)
{
    if (!v || stream >= v->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(v->e->mtx);
    if (const int rc = enter(v->e)) return rc;
    return damaged_guards({{v->ring, stream}, {v->cnt, 0}, {v->out, 0}});
}

}  // extern "C"

/* ---------------------------------------------------------------- Horus Binary 4FSK (kernels/fsk4.hip) --------------------------------- */

struct hd_fsk4 {
    static constexpr const char* kNull = "null fsk4 object";
    hd_engine* e = nullptr;
    hd_fsk4_params prm{};
    uint32_t S = 0, slot_cap = 0;
    DevBuf<hd::Fsk4State> st;                    // [S]
    Guarded<uint32_t> ring32;                    // [S * 8]: guard | kFsk4Ring32 running sums | guard
    Guarded<uint32_t> slots;                     // [S]: guard | slot_cap records of four words | guard
    Guarded<uint32_t> cnt;                       // one row: guard | the launch's candidates behind the gate (and three words unused) | guard
    Guarded<uint32_t> out;                       // one row: guard | HD_FSK4_LAUNCH results (hd::Fsk4Out) | guard
    DevBuf<hd::Fsk4Tab> tab;                     // [S]
    DevBuf<int32_t> ctab;                        // [1024]
    DevBuf<float2> slab;                         // hd_fsk4_push_host: the rows packed end to end, grown on demand
    PinBuf<hd::TonesSrc> src;                    // [S]: a slot launch's descriptors, read by the kernel in place (a launch is waited for before the next is written)
    PinBuf<hd::Fsk4Cand> cand;                   // [S]: a frame launch's
    std::vector<hd::Fsk4Stream> stream;          // [S]: the modem (s: the state a reset gives, with n and g as the device has them), the frame's tables,
                                                 // selection, delivery and counters
    std::vector<hd::Fsk4Out> h_out, found;       // a launch's results; a scan's
    uint64_t pushed_calls = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;       // set by the measurement hook only: recorded around the slot launches of a push ...
    hipEvent_t f0 = nullptr, f1 = nullptr;       // ... and around the frame launches of its scan
    bool frames_launched = false;
    std::vector<uint32_t> done;                  // launch_rounds' scratch
};
// (the strides the kernels were written against, fsk4.h)
static_assert(Guarded<uint32_t>::stride_of(hd::kFsk4Ring32, hd::kFsk4Guard) == hd::kFsk4Ring32 + 2 * hd::kFsk4Guard, "fsk4 ring stride");
static_assert(sizeof(hd::Fsk4Out) == 64 && sizeof(hd::Fsk4Tab) % 16 == 0, "fsk4 result and table layout");

namespace {

constexpr size_t kFsk4OutWords = sizeof(hd::Fsk4Out) / sizeof(uint32_t);

// launch_chunks over the frame launch's descriptors: the object's engine and streams, `cand` under the name the helper knows, the scan's two events.
struct Fsk4FrameLaunches {
    hd_engine* e;
    uint32_t S;
    PinBuf<hd::Fsk4Cand>& src;
    hipEvent_t t0, t1;
};

// Every candidate whose last slot exists and is not decided: at most HD_FSK4_LAUNCH over all streams per launch, so that the results of a launch always
// fit.  The results are sorted by (stream, slot) before they meet the selection -- what a scan delivers cannot depend on the order in which waves
// finished.  Every slot a candidate reads is in the ring: fsk4_slot_cap.
int fsk4_scan(hd_fsk4* f)
{
    hipStream_t q = f->e->qa;
    f->found.clear();
    f->frames_launched = false;
    uint32_t max_cand = 0, active = 0;
    for (uint32_t s = 0; s < f->S; ++s) {
        const hd::Fsk4Stream& st = f->stream[s];
        hd::Fsk4Cand& d = f->cand.p[s];
        d.base = st.decided;
        d.n_total = (uint32_t)std::min<uint64_t>(st.decidable(st.s.g), f->slot_cap);
        d.off = 0; d.n = 0;
        max_cand = std::max(max_cand, d.n_total);
        active += d.n_total != 0;
    }
    if (!max_cand) return HD_OK;
    uint32_t cap = 0;
    hipError_t fetch = hipSuccess;
    Fsk4FrameLaunches view{f->e, f->S, f->cand, f->f0, f->f1};
    const int rc = launch_chunks(
        &view, max_cand, std::max(1u, (uint32_t)HD_FSK4_LAUNCH / active), "",
        [&](uint32_t, const hd::Fsk4Cand& d) { cap = std::max(cap, d.n); },
        [&] {
            if (hipMemsetAsync(f->cnt.row(0), 0, 4 * sizeof(uint32_t), q) != hipSuccess) return false;
            hd::launch_fsk4_frames(q, f->S, cap, f->cand.dev, f->tab.p, f->slots.base(), f->slots.stride, f->slot_cap, f->prm.uw_max_errors, f->prm.chase_bits,
                                   f->cnt.row(0), reinterpret_cast<hd::Fsk4Out*>(f->out.row(0)), HD_FSK4_LAUNCH);
            cap = 0;
            return true;
        },
        [&] {                                    // the launch is done: its count, and its results if it has any
            if (fetch != hipSuccess) return;
            uint32_t k = 0;
            fetch = hipMemcpy(&k, f->cnt.row(0), sizeof k, hipMemcpyDeviceToHost);
            k = std::min<uint32_t>(k, HD_FSK4_LAUNCH);
            if (fetch != hipSuccess || !k) return;
            fetch = hipMemcpy(f->h_out.data(), f->out.row(0), k * sizeof(hd::Fsk4Out), hipMemcpyDeviceToHost);
            if (fetch == hipSuccess) f->found.insert(f->found.end(), f->h_out.begin(), f->h_out.begin() + k);
        });
    if (rc) return rc;
    HD_HIP(fetch);
    f->frames_launched = true;
    std::sort(f->found.begin(), f->found.end(), [](const hd::Fsk4Out& a, const hd::Fsk4Out& b) { return a.stream != b.stream ? a.stream < b.stream : a.slot < b.slot; });
    for (const hd::Fsk4Out& r : f->found)
        if (r.stream < f->S) f->stream[r.stream].accept(r);
    for (uint32_t s = 0; s < f->S; ++s) f->stream[s].decided_more(f->cand.p[s].n_total);
    return HD_OK;
}

// The tones a retune put in force go to the device: phi and psi lie together in the state.  On the queue, in front of the next launch.
hipError_t fsk4_copy_tones(hd_fsk4* f, uint32_t s)
{
    return hipMemcpyAsync(reinterpret_cast<char*>(f->st.p + s) + offsetof(hd::Fsk4State, phi), f->stream[s].s.phi, 8 * sizeof(uint32_t), hipMemcpyHostToDevice,
                          f->e->qa);
}

// Its own: a stream without a modem is passed by, in front of the max_push test.  Round by round (launch_rounds): a stream's retunes whose sample has come
// take effect and its new tones are copied on the queue; the launch takes the stream's samples up to the next waiting retune, HD_FSK4_CHUNK at most;
// `cap`, the longest part of a row in the launch, sizes its LDS; behind the wait the host's copy of n and g follows the device's.  Then the scan.
int fsk4_launch(hd_fsk4* f, uint32_t max_n)
{
    if (const int rc = check_max_push(f, "hd_fsk4", &max_n, [f](uint32_t s) { if (!f->stream[s].s.F) f->src.p[s].n_total = 0; })) return rc;
    uint32_t cap = 0;
    hipError_t copy = hipSuccess;                // of a retuned stream's tones; a failure ends the push behind the round's wait, with HIP's own message
    const int rc = launch_rounds(
        f, "fsk4: the launch's chunk does not fit the LDS",
        [&](uint32_t s, hd::TonesSrc&, uint32_t left) {
            hd::Fsk4Stream& st = f->stream[s];
            if (!st.pending.empty() && st.apply_retunes() && copy == hipSuccess) copy = fsk4_copy_tones(f, s);
            const uint32_t n = (uint32_t)st.uncut(std::min<uint32_t>(left, HD_FSK4_CHUNK));
            cap = std::max(cap, n);
            return n;
        },
        [&] {
            const uint32_t longest = cap;
            cap = 0;
            return hd::launch_fsk4_slots(f->e->qa, f->S, longest, f->src.dev, f->st.p, f->ring32.base(), f->ring32.stride, f->ctab.p, f->slots.base(),
                                         f->slots.stride, f->slot_cap);
        },
        [&]() -> int {
            for (uint32_t s = 0; s < f->S; ++s) {
                hd::Fsk4State& m = f->stream[s].s;
                if (!m.F || !f->src.p[s].n) continue;
                m.n += f->src.p[s].n;
                m.g = hd::fsk4_slots_before(m.F, m.n);
            }
            HD_HIP(copy);
            return HD_OK;
        });
    if (rc) return rc;
    return fsk4_scan(f);
}

// (The rings need no clearing: nothing in front of a stream's index 0 is read, and no candidate reads a slot that was not written since.)
int fsk4_clear(hd_fsk4* f, uint32_t s0, uint32_t ns)
{
    hipStream_t q = f->e->qa;
    for (uint32_t s = s0; s < s0 + ns; ++s) {
        f->stream[s].reset();
        HD_HIP(hipMemcpyAsync(f->st.p + s, &f->stream[s].s, sizeof(hd::Fsk4State), hipMemcpyHostToDevice, q));
    }
    HD_HIP(hipStreamSynchronize(q));
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_fsk4_params_default(hd_fsk4_params* p) { if (p) hd::fsk4_params_default(p); }

int hd_fsk4_create(hd_engine* e, const hd_fsk4_params* params, hd_fsk4** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_fsk4> f(new hd_fsk4);
    f->e = e; f->S = e->S;
    hd::fsk4_params_default(&f->prm);
    if (params) f->prm = *params;
    if (!hd::fsk4_window_ok(f->prm.window_q8)) return fail(HD_ERR_UNSUPPORTED, "fsk4 parameters: 32 <= window_q8 <= 256");
    if (!hd::fsk4_params_ok(&f->prm)) return fail(HD_ERR_INVALID, "fsk4 parameters: uw_max_errors <= 4, chase_bits <= 6, max_push <= 2^22");
    // (a launch takes at least one candidate of every active stream and its results must fit HD_FSK4_LAUNCH slots)
    if (e->S > HD_FSK4_LAUNCH) return fail(HD_ERR_UNSUPPORTED, "hd_fsk4_create: at most " + std::to_string(HD_FSK4_LAUNCH) + " streams");
    if (const int rc = default_max_push(e, &f->prm.max_push, "fsk4")) return rc;
    if (f->prm.max_push > (1u << 22)) return fail(HD_ERR_INVALID, "fsk4 parameters: max_push <= 2^22");
    if (const int rc = enter(e)) return rc;
    const uint32_t S = f->S;
    f->slot_cap = hd::fsk4_slot_cap(f->prm.max_push);
    f->stream.resize(S);
    for (auto& st : f->stream) st.set_params(f->prm);
    f->h_out.resize(HD_FSK4_LAUNCH);
    int32_t C[1024];
    hd::tones_table(C);
    HD_HIP(f->st.alloc_unfilled(S));
    HD_HIP(f->ring32.alloc((size_t)S * 8, hd::kFsk4Ring32, hd::kFsk4Guard, hd::kFsk4GuardWord, e->qa));
    HD_HIP(f->slots.alloc(S, (size_t)f->slot_cap * 4, hd::kFsk4Guard, hd::kFsk4GuardWord, e->qa));
    HD_HIP(f->cnt.alloc(1, 4, hd::kFsk4Guard, hd::kFsk4GuardWord, e->qa));
    HD_HIP(f->out.alloc(1, (size_t)HD_FSK4_LAUNCH * kFsk4OutWords, hd::kFsk4Guard, hd::kFsk4GuardWord, e->qa));
    HD_HIP(f->tab.alloc(S));
    HD_HIP(f->ctab.alloc_unfilled(1024));
    HD_HIP(f->src.alloc(S));
    HD_HIP(f->cand.alloc(S));
    HD_HIP(hipMemcpyAsync(f->ctab.p, C, sizeof C, hipMemcpyHostToDevice, e->qa));
    if (const int rc = fsk4_clear(f.get(), 0, S)) return rc;           // (waits for the queue: `C` is a local)
    *out = f.release();
    return HD_OK;
}

void hd_fsk4_destroy(hd_fsk4* f) { destroy(f); }

int hd_fsk4_reset(hd_fsk4* f, uint32_t stream) { return reset(f, stream, fsk4_clear); }

int hd_fsk4_set_modem(hd_fsk4* f, uint32_t stream, double baud, double f0_hz, double spacing_hz, const hd_fsk4_frame* frame)
{
    if (const int rc = check_object(f, stream)) return rc;
    if (!frame) return fail(HD_ERR_INVALID, "null frame");
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    std::unique_ptr<hd::Fsk4Tab> tab(new hd::Fsk4Tab);
    if (!hd::fsk4_tables(*frame, *tab))
        return fail(HD_ERR_UNSUPPORTED, "fsk4: a frame the decoder cannot take (3 <= payload_bytes <= 32, interleave_mul coprime with the body's bits, a nonzero 15-bit seed, a Golay generator)");
    hd::Fsk4State m;
    const int rc = hd::fsk4_modem(m, f->e->fsd, baud, f0_hz, spacing_hz, f->prm.window_q8);
    if (rc == HD_ERR_UNSUPPORTED) return fail(rc, "fsk4: 8 <= decimated rate / baud <= " + std::to_string(HD_FSK4_MAX_SPB));
    if (rc) return fail(rc, "fsk4: every tone f0 + t spacing, t = 0 .. 3, inside +- decimated rate / 2");
    if (const int rc2 = enter(f->e)) return rc2;
    hd::Fsk4Stream& st = f->stream[stream];
    st.s = m; st.tab = *tab;
    HD_HIP(hipMemcpyAsync(f->tab.p + stream, &st.tab, sizeof(hd::Fsk4Tab), hipMemcpyHostToDevice, f->e->qa));
    return fsk4_clear(f, stream, 1);
}

int hd_fsk4_push_engine(hd_fsk4* f) { return push_engine(f, "hd_fsk4_push_engine", fsk4_launch); }

int hd_fsk4_push_device(hd_fsk4* f, const float* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(f, reinterpret_cast<const float2*>(d_iq), stride, n_per_stream, n, true, fsk4_launch);
}

int hd_fsk4_push_host(hd_fsk4* f, const float* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(f, reinterpret_cast<const float2*>(iq), stride, n_per_stream, n, false, fsk4_launch);
}

int hd_fsk4_scan(hd_fsk4* f)
{
    if (!f) return fail(HD_ERR_INVALID, hd_fsk4::kNull);
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    if (const int rc = enter(f->e)) return rc;
    return fsk4_scan(f);
}

int hd_fsk4_take_frames(hd_fsk4* f, uint32_t stream, hd_fsk4_rx* out, size_t cap)
{
    if (const int rc = check_object(f, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    if (const int rc = enter(f->e)) return rc;
    return (int)f->stream[stream].take(out, cap);
}

// (samples and slots are the device's own: a host copy that had drifted would show here)
int hd_fsk4_stats(hd_fsk4* f, uint32_t stream, hd_fsk4_counters* out)
{
    if (const int rc = check_object(f, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    if (const int rc = enter(f->e)) return rc;
    hd::Fsk4State h;
    HD_HIP(hipMemcpy(&h, f->st.p + stream, sizeof h, hipMemcpyDeviceToHost));
    f->stream[stream].stats(out, h.n, h.g);
    return HD_OK;
}

int hd_fsk4_retune(hd_fsk4* f, uint32_t stream, double f0_hz, double spacing_hz, uint64_t at_sample)
{
    if (const int rc = check_object(f, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    if (const int rc = enter(f->e)) return rc;
    hd::Fsk4Stream& st = f->stream[stream];
    if (!st.s.F) return fail(HD_ERR_INVALID, "hd_fsk4_retune: the stream has no modem");
    uint32_t phi[4];
    if (hd::fsk4_retune_steps(f->e->fsd, f0_hz, spacing_hz, phi)) return fail(HD_ERR_INVALID, "fsk4: every tone f0 + t spacing, t = 0 .. 3, inside +- decimated rate / 2");
    st.retune(phi, at_sample);
    if (st.apply_retunes()) {                     // its sample has come already: at once
        HD_HIP(fsk4_copy_tones(f, stream));
        HD_HIP(hipStreamSynchronize(f->e->qa));
    }
    return HD_OK;
}

int hd_fsk4_retune_stats(hd_fsk4* f, uint32_t stream, hd_fsk4_retune_info* out)
{
    if (const int rc = check_object(f, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    if (const int rc = enter(f->e)) return rc;
    hd::Fsk4State h;
    HD_HIP(hipMemcpy(&h, f->st.p + stream, sizeof h, hipMemcpyDeviceToHost));
    const hd::Fsk4Stream& st = f->stream[stream];
    *out = hd_fsk4_retune_info{st.retunes, st.late, st.pending.size(), {h.psi[0], h.psi[1], h.psi[2], h.psi[3]}};
    return HD_OK;
}

// The measurement hook (tools/micro/fsk4_rate.py; not part of the ABI): hd_fsk4_push_engine with the slot launches and the frame launches of its scan
// each between two HIP events (0 where none was launched), and the host time of the whole call in microseconds.
int hd_debug_fsk4_push_timed(hd_fsk4* f, float* slots_ms, float* frames_ms, double* host_us)
{
    if (!f || !slots_ms || !frames_ms || !host_us) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    if (const int rc = enter(f->e)) return rc;
    HD_HIP(hipEventCreate(&f->f0));
    HD_HIP(hipEventCreate(&f->f1));
    f->frames_launched = false;
    const int rc = push_timed(f, slots_ms, host_us, hd_fsk4_push_engine);
    *frames_ms = 0;
    if (rc == HD_OK && f->frames_launched && hipEventQuery(f->f1) == hipSuccess) (void)hipEventElapsedTime(frames_ms, f->f0, f->f1);
    (void)hipGetLastError();
    (void)hipEventDestroy(f->f0); (void)hipEventDestroy(f->f1);
    f->f0 = f->f1 = nullptr;
    return rc;
}

// Test hooks (tests/test_gpu_fsk4.py; not part of the ABI).  The records of the slots first .. first + n - 1 as the stream's ring holds them, 4 n words.
int hd_debug_fsk4_slots(hd_fsk4* f, uint32_t stream, uint64_t first, uint32_t* out, size_t n)
{
    if (!f || stream >= f->S || !out || n > f->slot_cap) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    if (const int rc = enter(f->e)) return rc;
    for (size_t k = 0; k < n;) {
        const size_t at = (size_t)((first + k) & (f->slot_cap - 1u)), run = std::min<size_t>(n - k, f->slot_cap - at);
        HD_HIP(hipMemcpy(out + 4 * k, f->slots.row(stream) + 4 * at, run * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        k += run;
    }
    return (int)n;
}

// The log of the stream's candidates behind the unique-word gate, as hd_host_fsk4_candidates.
int hd_debug_fsk4_candidates(hd_fsk4* f, uint32_t stream, hd_fsk4_candidate* out, size_t cap)
{
    if (!f || stream >= f->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    return (int)f->stream[stream].take_log(out, cap);
}

// How many of the guard words around the stream's eight rings and its slots, the count and the results no longer hold their pattern.
int hd_debug_fsk4_guards(hd_fsk4* f, uint32_t stream)
{
    if (!f || stream >= f->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(f->e->mtx);
    if (const int rc = enter(f->e)) return rc;
    const size_t r = (size_t)stream * 8;
    return damaged_guards({{f->ring32, r}, {f->ring32, r + 1}, {f->ring32, r + 2}, {f->ring32, r + 3}, {f->ring32, r + 4}, {f->ring32, r + 5},
                           {f->ring32, r + 6}, {f->ring32, r + 7}, {f->slots, stream}, {f->cnt, 0}, {f->out, 0}});
}

}  // extern "C"

/* ---------------------------------------------------------------- 4FSK tone tracker (kernels/fsk4_track.hip) --------------------------- */

struct hd_fsk4_track {
    static constexpr const char* kNull = "null fsk4 tracker";
    hd_engine* e = nullptr;
    hd_fsk4_track_params prm{};
    uint32_t S = 0;
    Guarded<double> acc;                         // [S]: guard | 4096 fftshifted sums | guard -- the tone search's layout, this object's own sums
    Guarded<float2> carry;                       // [S * 2]: the tone search's two carry buffers per stream
    Guarded<uint32_t> rec;                       // [S]: guard | the 16 words of the stream's newest record | guard
    DevBuf<float> win;                           // [4096] the survey's window table
    DevBuf<float2> own_tw;                       // the twiddles where the engine computes no spectra and holds none
    const float2* tw = nullptr;
    DevBuf<float2> slab;                         // hd_fsk4_track_push_host: the rows packed end to end, grown on demand
    PinBuf<hd::ToneSearchSrc> src;               // [S]: a spectrum launch's descriptors
    PinBuf<hd::Fsk4CombSrc> comb;                // [S]: a comb launch's
    std::vector<hd::Fsk4TrackBook> book;         // [S]: the stream's search, epochs, counts and records
    std::vector<uint32_t> carry_n, flip;         // [S]: the carry's length, and which of the two buffers holds it
    std::vector<uint32_t> done;                  // launch_rounds' scratch
    std::vector<hd_fsk4_comb_record> h_rec;      // [S]: a comb launch's records
    hd_fsk4* modem = nullptr;                    // attached: retuned at epoch ends
    uint64_t pushed_calls = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;       // set by the measurement hook only: recorded around the launches of a push ...
    hipEvent_t c0 = nullptr, c1 = nullptr;       // ... and around each comb launch, whose times add up in comb_ms
    float comb_ms = 0;
};
static_assert(sizeof(hd_fsk4_comb_record) == 64, "the comb record is 16 words");
static_assert(Guarded<double>::stride_of(hd::kFsk4CombBins, hd::kFsk4TrackGuard) == hd::kToneSearchSeg + hd::kToneSearchGuard && hd::kFsk4TrackGuard == hd::kToneSearchGuard,
              "the tracker's sums and carries have the tone search's layout: its kernel writes them");

namespace {

// One comb launch over the streams whose descriptor says due, waited for; the records of all streams come back (a stream that was not due keeps its last).
int fsk4_track_comb(hd_fsk4_track* tr)
{
    hipStream_t q = tr->e->qa;
    std::atomic_thread_fence(std::memory_order_release);
    if (tr->c0) HD_HIP(hipEventRecord(tr->c0, q));
    hd::launch_fsk4_comb(q, tr->S, tr->comb.dev, tr->acc.base(), tr->acc.stride, tr->rec.base(), tr->rec.stride);
    HD_HIP(hipGetLastError());
    if (tr->c1) HD_HIP(hipEventRecord(tr->c1, q));
    if (tr->t1) HD_HIP(hipEventRecord(tr->t1, q));                     // (the push's last launch so far)
    HD_HIP(hipStreamSynchronize(q));
    if (tr->c1) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, tr->c0, tr->c1) == hipSuccess) tr->comb_ms += ms;
    }
    HD_HIP(hipMemcpy2D(tr->h_rec.data(), sizeof(hd_fsk4_comb_record), tr->rec.row(0), tr->rec.stride * sizeof(uint32_t), sizeof(hd_fsk4_comb_record), tr->S,
                       hipMemcpyDeviceToHost));
    return HD_OK;
}

// Its own: a stream without a search is passed by, in front of the max_push test.  Round by round (launch_rounds): the spectrum launch -- the tone search's,
// with its descriptor -- takes a stream's samples up to its epoch's end, HD_TONE_SEARCH_CHUNK at most; behind the wait the counts move on, and where
// an epoch ended the comb launch follows, its records join the streams' logs and an attached modem is retuned.
int fsk4_track_launch(hd_fsk4_track* tr, uint32_t max_n)
{
    if (const int rc = check_max_push(tr, "hd_fsk4_track", &max_n, [tr](uint32_t s) { if (!tr->book[s].set) tr->src.p[s].n_total = 0; })) return rc;
    const uint32_t E = tr->prm.epoch_segments;
    return launch_rounds(
        tr, "",
        [&](uint32_t s, hd::ToneSearchSrc& d, uint32_t left) {
            const uint32_t n = (uint32_t)tr->book[s].uncut(std::min<uint32_t>(left, HD_TONE_SEARCH_CHUNK), E);
            d.carry = tr->carry_n[s];
            d.segs = hd::tone_search_segments(d.carry, n);
            d.flip = tr->flip[s];
            return n;
        },
        [&] {
            hd::launch_tone_search(tr->e->qa, tr->S, tr->src.dev, tr->win.p, tr->tw, tr->acc.base(), tr->acc.stride, tr->carry.base(), tr->carry.stride);
            return true;
        },
        [&]() -> int {
            bool any = false;
            for (uint32_t s = 0; s < tr->S; ++s) {
                const hd::ToneSearchSrc& d = tr->src.p[s];
                hd::Fsk4CombSrc& c = tr->comb.p[s];
                c.due = 0;
                if (!d.n) continue;
                hd::Fsk4TrackBook& b = tr->book[s];
                b.samples += d.n;
                b.segments += d.segs;
                tr->carry_n[s] = d.carry + d.n - d.segs * hd::kToneSearchStep;
                if (d.segs) tr->flip[s] ^= 1u;
                if (b.samples != b.epoch_end(E)) continue;
                c.plan = b.plan; c.due = 1; c.min_quality_q8 = tr->prm.min_quality_q8; c.segments_ok = b.segments_ok(tr->prm); c.decay_q8 = tr->prm.decay_q8;
                any = true;
            }
            if (!any) return HD_OK;
            if (const int rc = fsk4_track_comb(tr)) return rc;
            for (uint32_t s = 0; s < tr->S; ++s) {
                if (!tr->comb.p[s].due) continue;
                hd::Fsk4TrackBook& b = tr->book[s];
                const hd_fsk4_track_est est = b.close_epoch(tr->h_rec[s], tr->prm, tr->e->fsd);
                if (!tr->modem || !tr->modem->stream[s].s.F) continue;
                if (!b.wants_retune(est, hd::fsk4_steps_ahead(tr->modem->stream[s]), tr->e->fsd, tr->prm.deadband)) continue;
                uint32_t phi[4];
                if (hd::fsk4_retune_steps(tr->e->fsd, est.f0_hz, est.spacing_hz, phi)) continue;      // a tone out of band: no retune, and no error either
                if (const int rc = hd_fsk4_retune(tr->modem, s, est.f0_hz, est.spacing_hz, est.end_sample)) return rc;
                ++b.retunes;
            }
            return HD_OK;
        });
}

// (The carry buffers need no clearing: nothing behind a stream's carry length is read.)
int fsk4_track_clear(hd_fsk4_track* tr, uint32_t s0, uint32_t ns)
{
    hipStream_t q = tr->e->qa;
    HD_HIP(hipMemset2DAsync(tr->acc.row(s0), tr->acc.stride * sizeof(double), 0, (size_t)hd::kFsk4CombBins * sizeof(double), ns, q));
    HD_HIP(hipMemset2DAsync(tr->rec.row(s0), tr->rec.stride * sizeof(uint32_t), 0, sizeof(hd_fsk4_comb_record), ns, q));
    HD_HIP(hipStreamSynchronize(q));
    for (uint32_t s = s0; s < s0 + ns; ++s) { tr->book[s].reset(); tr->carry_n[s] = tr->flip[s] = 0; }
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_fsk4_track_params_default(hd_fsk4_track_params* p) { if (p) hd::fsk4_track_params_default(p); }

int hd_fsk4_track_create(hd_engine* e, const hd_fsk4_track_params* params, hd_fsk4_track** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_fsk4_track> tr(new hd_fsk4_track);
    tr->e = e; tr->S = e->S;
    hd::fsk4_track_params_default(&tr->prm);
    if (params) tr->prm = *params;
    if (!hd::fsk4_track_params_ok(&tr->prm)) return fail(HD_ERR_INVALID, "fsk4 tracker parameters: 1 <= epoch_segments <= 4096, decay_q8 <= 256");
    if (const int rc = default_max_push(e, &tr->prm.max_push, "fsk4 tracker")) return rc;
    if (const int rc = enter(e)) return rc;
    const uint32_t S = tr->S;
    tr->book.resize(S); tr->carry_n.assign(S, 0u); tr->flip.assign(S, 0u); tr->h_rec.resize(S);
    std::vector<float> w(hd::kToneSearchSeg);
    hd::survey_window(w.data());
    std::vector<float2> tw_host;
    HD_HIP(tr->acc.alloc(S, hd::kFsk4CombBins, hd::kFsk4TrackGuard, hd::kFsk4TrackGuardWord, e->qa));
    HD_HIP(tr->carry.alloc((size_t)S * 2, hd::kToneSearchSeg, hd::kFsk4TrackGuard, hd::kFsk4TrackGuardWord, e->qa));
    HD_HIP(tr->rec.alloc(S, sizeof(hd_fsk4_comb_record) / sizeof(uint32_t), hd::kFsk4TrackGuard, hd::kFsk4TrackGuardWord, e->qa));
    HD_HIP(tr->win.alloc_unfilled(w.size()));
    HD_HIP(tr->src.alloc(S));
    HD_HIP(tr->comb.alloc(S));
    if (const int rc = hd::eng::engine_or_own_twiddles(e, tr->own_tw, tw_host, e->qa, &tr->tw)) return rc;
    HD_HIP(hipMemcpyAsync(tr->win.p, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, e->qa));
    if (const int rc = fsk4_track_clear(tr.get(), 0, S)) return rc;    // (waits for the queue: the tables are locals)
    *out = tr.release();
    return HD_OK;
}

void hd_fsk4_track_destroy(hd_fsk4_track* tr) { destroy(tr); }

int hd_fsk4_track_reset(hd_fsk4_track* tr, uint32_t stream) { return reset(tr, stream, fsk4_track_clear); }

int hd_fsk4_track_set_stream(hd_fsk4_track* tr, uint32_t stream, double baud, double spacing_lo_hz, double spacing_hi_hz, double f_lo_hz, double f_hi_hz)
{
    if (const int rc = check_object(tr, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(tr->e->mtx);
    hd::Fsk4CombPlan pl;
    const int rc = hd::fsk4_comb_plan(tr->e->fsd, baud, spacing_lo_hz, spacing_hi_hz, f_lo_hz, f_hi_hz, pl);
    if (rc == HD_ERR_UNSUPPORTED) return fail(rc, "fsk4 tracker: a tone spacing below 2 baud is not searched");
    if (rc) return fail(rc, "fsk4 tracker: baud > 0, 0 < spacing_lo_hz <= spacing_hi_hz, f_lo_hz < f_hi_hz, and a band that holds the narrowest comb");
    if (const int rc2 = enter(tr->e)) return rc2;
    tr->book[stream].plan = pl; tr->book[stream].baud = baud; tr->book[stream].set = true;
    return fsk4_track_clear(tr, stream, 1);
}

int hd_fsk4_track_attach(hd_fsk4_track* tr, hd_fsk4* f)
{
    if (!tr) return fail(HD_ERR_INVALID, hd_fsk4_track::kNull);
    if (f && f->e != tr->e) return fail(HD_ERR_INVALID, "hd_fsk4_track_attach: the fsk4 object belongs to another engine");
    std::lock_guard<std::recursive_mutex> lock(tr->e->mtx);
    tr->modem = f;
    return HD_OK;
}

int hd_fsk4_track_push_engine(hd_fsk4_track* tr) { return push_engine(tr, "hd_fsk4_track_push_engine", fsk4_track_launch); }

int hd_fsk4_track_push_device(hd_fsk4_track* tr, const float* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(tr, reinterpret_cast<const float2*>(d_iq), stride, n_per_stream, n, true, fsk4_track_launch);
}

int hd_fsk4_track_push_host(hd_fsk4_track* tr, const float* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(tr, reinterpret_cast<const float2*>(iq), stride, n_per_stream, n, false, fsk4_track_launch);
}

int hd_fsk4_track_estimate(hd_fsk4_track* tr, uint32_t stream, hd_fsk4_track_est* out)
{
    if (const int rc = check_object(tr, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(tr->e->mtx);
    if (tr->book[stream].log.empty()) return fail(HD_ERR_UNSUPPORTED, "hd_fsk4_track_estimate: no epoch of the stream has ended");
    *out = tr->book[stream].log.back();
    return HD_OK;
}

int hd_fsk4_track_stats(hd_fsk4_track* tr, uint32_t stream, hd_fsk4_track_info* out)
{
    if (const int rc = check_object(tr, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(tr->e->mtx);
    tr->book[stream].stats(out);
    return HD_OK;
}

// The measurement hook (tools/micro/fsk4_track_rate.py; not part of the ABI): hd_fsk4_track_push_engine between two HIP events -- the spectrum launches,
// the comb launches and the waits between them -- the comb launches alone (0 where no epoch ended), and the host time of the whole call in microseconds.
int hd_debug_fsk4_track_push_timed(hd_fsk4_track* tr, float* push_ms, float* comb_ms, double* host_us)
{
    if (!tr || !push_ms || !comb_ms || !host_us) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(tr->e->mtx);
    if (const int rc = enter(tr->e)) return rc;
    HD_HIP(hipEventCreate(&tr->c0));
    HD_HIP(hipEventCreate(&tr->c1));
    tr->comb_ms = 0;
    const int rc = push_timed(tr, push_ms, host_us, hd_fsk4_track_push_engine);
    *comb_ms = tr->comb_ms;
    (void)hipEventDestroy(tr->c0); (void)hipEventDestroy(tr->c1);
    tr->c0 = tr->c1 = nullptr;
    return rc;
}

// Test hooks (tests/test_gpu_fsk4_track.py; not part of the ABI).  All records of the stream since its last reset, oldest first (the log keeps the newest
// 4096); out null: how many.
int hd_debug_fsk4_track_records(hd_fsk4_track* tr, uint32_t stream, hd_fsk4_track_est* out, size_t cap)
{
    if (!tr || stream >= tr->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(tr->e->mtx);
    return (int)tr->book[stream].take_log(out, cap, true);
}

// The stream's 4096 sums as they lie in device memory.
int hd_debug_fsk4_track_acc(hd_fsk4_track* tr, uint32_t stream, double* out)
{
    if (!tr || stream >= tr->S || !out) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(tr->e->mtx);
    if (const int rc = enter(tr->e)) return rc;
    HD_HIP(hipMemcpy(out, tr->acc.row(stream), hd::kFsk4CombBins * sizeof(double), hipMemcpyDeviceToHost));
    return (int)hd::kFsk4CombBins;
}

// One comb launch over spectra of the test's making: spectra [S][4096] replace the streams' sums, stream s is searched by its own plan where due[s] is
// set (with segments_ok[s] and the object's min_quality_q8 and decay_q8), and the records of all streams come back.  The streams want a reset afterwards.
int hd_debug_fsk4_track_comb(hd_fsk4_track* tr, const double* spectra, const uint32_t* due, const uint32_t* segments_ok, hd_fsk4_comb_record* out)
{
    if (!tr || !spectra || !due || !segments_ok || !out) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(tr->e->mtx);
    if (const int rc = enter(tr->e)) return rc;
    for (uint32_t s = 0; s < tr->S; ++s)
        if (due[s] && !tr->book[s].set) return fail(HD_ERR_INVALID, "hd_debug_fsk4_track_comb: a due stream without a search");
    HD_HIP(hipMemcpy2D(tr->acc.row(0), tr->acc.stride * sizeof(double), spectra, hd::kFsk4CombBins * sizeof(double), hd::kFsk4CombBins * sizeof(double), tr->S,
                       hipMemcpyHostToDevice));
    for (uint32_t s = 0; s < tr->S; ++s) {
        hd::Fsk4CombSrc& c = tr->comb.p[s];
        c.plan = tr->book[s].plan; c.due = due[s] ? 1u : 0u; c.min_quality_q8 = tr->prm.min_quality_q8; c.segments_ok = segments_ok[s] ? 1u : 0u;
        c.decay_q8 = tr->prm.decay_q8;
    }
    if (const int rc = fsk4_track_comb(tr)) return rc;
    std::memcpy(out, tr->h_rec.data(), (size_t)tr->S * sizeof(hd_fsk4_comb_record));
    return HD_OK;
}

// How many of the guard words around the stream's sums, its two carry buffers and its record no longer hold their pattern.
int hd_debug_fsk4_track_guards(hd_fsk4_track* tr, uint32_t stream)
{
    if (!tr || stream >= tr->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(tr->e->mtx);
    if (const int rc = enter(tr->e)) return rc;
    return damaged_guards({{tr->acc, stream}, {tr->carry, (size_t)stream * 2}, {tr->carry, (size_t)stream * 2 + 1}, {tr->rec, stream}});
}

}  // extern "C"

/* ---------------------------------------------------------------- AFSK / AX.25 (kernels/afsk.hip) -------------------------------------- */

struct hd_afsk {
    static constexpr const char* kNull = "null afsk object";
    hd_engine* e = nullptr;
    hd_afsk_params prm{};
    uint32_t S = 0;
    DevBuf<hd::AfskState> st;                    // [S]
    Guarded<uint32_t> ring32;                    // [S * 4]: guard | kAfskRing32 running sums | guard
    Guarded<int32_t> slots;                      // [S]: guard | HD_AFSK_RING records | guard
    Guarded<uint32_t> count;                     // one row: guard | a scan's flags per stream [S] | guard
    Guarded<uint32_t> list;                      // [S]: guard | kListCap offsets of the scan's flags | guard
    Guarded<uint32_t> out;                       // one row: guard | HD_AFSK_LAUNCH results (hd_afsk_candidate) | guard
    DevBuf<hd::AfskPatterns> pat;                // [1]
    DevBuf<int32_t> ctab;                        // [1024]
    DevBuf<float> slab;                          // hd_afsk_push_host: the rows packed end to end, grown on demand
    PinBuf<hd::ClockedSrc> src;                  // [S]: a slot launch's descriptors, read by the kernel in place (a launch is waited for before the next is written)
    PinBuf<hd::AfskGate> gate;                   // [S]: the gate launch's
    PinBuf<hd::AfskCand> cand;                   // [S]: a frame launch's
    std::vector<hd::AfskStream> stream;          // [S]: the modem (s: the state a reset gives, with n and g as the device has them), selection, delivery, counters
    std::vector<uint32_t> h_count;               // [S]
    std::vector<hd_afsk_candidate> h_out;        // a launch's results
    uint64_t pushed_calls = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;       // set by the measurement hook only: recorded around the slot launches of a push ...
    hipEvent_t f0 = nullptr, f1 = nullptr;       // ... and around the gate and the frame launches of its scan
    bool frames_launched = false;
    // A stream's list holds every flag a scan can find: flags of one phase lie at least seven bits apart, and a scan has at most HD_AFSK_RING slots.
    static constexpr uint32_t kListCap = HD_AFSK_RING / 4;
};
// (the strides the kernels were written against, afsk.h)
static_assert(Guarded<uint32_t>::stride_of(hd::kAfskRing32, hd::kAfskGuard) == hd::kAfskRing32 + 2 * hd::kAfskGuard, "afsk ring stride");
static_assert(sizeof(hd_afsk_candidate) == 384 && sizeof(hd_afsk_rx) == 392 && sizeof(hd::AfskCand) == 24, "afsk record layouts");
static_assert(hd_afsk::kListCap >= HD_AFSK_RING / 7 + 8, "the flag list holds a scan's flags");

namespace {

constexpr size_t kAfskOutWords = sizeof(hd_afsk_candidate) / sizeof(uint32_t);

// launch_chunks over the frame launch's descriptors: the object's engine and streams, `cand` under the name the helper knows, the scan's closing event.
struct AfskFrameLaunches {
    hd_engine* e;
    uint32_t S;
    PinBuf<hd::AfskCand>& src;
    hipEvent_t t0, t1;
};

// Every slot whose longest walk's last slot exists and is not decided.  The gate lists each stream's flags in slot order; the frame kernel takes them
// in launches of at most HD_AFSK_LAUNCH over all streams, a stream's part of a launch at a place the host gave it -- what a scan delivers cannot
// depend on the order in which waves finished.  Every slot a candidate reads is in the ring: afsk_params_check.
int afsk_scan(hd_afsk* a)
{
    hipStream_t q = a->e->qa;
    a->frames_launched = false;
    bool any = false;
    for (uint32_t s = 0; s < a->S; ++s) {
        const hd::AfskStream& st = a->stream[s];
        hd::AfskGate& d = a->gate.p[s];
        d.base = st.decided;
        d.n = (uint32_t)std::min<uint64_t>(st.decidable(st.s.g), HD_AFSK_RING);
        any |= d.n != 0;
    }
    if (!any) return HD_OK;
    std::atomic_thread_fence(std::memory_order_release);
    if (a->f0) HD_HIP(hipEventRecord(a->f0, q));
    hd::launch_afsk_gate(q, a->S, a->gate.dev, a->slots.base(), a->slots.stride, a->count.base(), a->list.base(), a->list.stride, hd_afsk::kListCap);
    HD_HIP(hipGetLastError());
    if (a->f1) HD_HIP(hipEventRecord(a->f1, q));
    HD_HIP(hipMemcpyAsync(a->h_count.data(), a->count.row(0), (size_t)a->S * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
    HD_HIP(hipStreamSynchronize(q));
    a->frames_launched = true;
    uint32_t max_cand = 0, active = 0;
    for (uint32_t s = 0; s < a->S; ++s) {
        hd::AfskCand& d = a->cand.p[s];
        d.base = a->gate.p[s].base;
        d.n_total = a->gate.p[s].n ? std::min<uint32_t>(a->h_count[s], hd_afsk::kListCap) : 0u;
        d.off = 0; d.n = 0; d.out_off = 0;
        max_cand = std::max(max_cand, d.n_total);
        active += d.n_total != 0;
    }
    if (max_cand) {
        uint32_t cap = 0, total = 0;
        hipError_t fetch = hipSuccess;
        AfskFrameLaunches view{a->e, a->S, a->cand, nullptr, a->f1};
        const int rc = launch_chunks(
            &view, max_cand, std::max(1u, (uint32_t)HD_AFSK_LAUNCH / active), "",
            [&](uint32_t, hd::AfskCand& d) { d.out_off = total; total += d.n; cap = std::max(cap, d.n); },
            [&] {
                hd::launch_afsk_frames(q, a->S, cap, a->cand.dev, a->pat.p, a->prm.require_addr, a->slots.base(), a->slots.stride, a->list.base(), a->list.stride,
                                       reinterpret_cast<hd_afsk_candidate*>(a->out.row(0)), HD_AFSK_LAUNCH);
                cap = 0;
                return true;
            },
            [&] {                                // the launch is done: its records, stream by stream in slot order
                const uint32_t k = std::min<uint32_t>(total, HD_AFSK_LAUNCH);
                total = 0;
                if (fetch != hipSuccess || !k) return;
                fetch = hipMemcpy(a->h_out.data(), a->out.row(0), (size_t)k * sizeof(hd_afsk_candidate), hipMemcpyDeviceToHost);
                if (fetch != hipSuccess) return;
                for (uint32_t s = 0; s < a->S; ++s) {
                    const hd::AfskCand& d = a->cand.p[s];
                    for (uint32_t i = 0; i < d.n && d.out_off + i < k; ++i) a->stream[s].accept(a->h_out[d.out_off + i]);
                }
            });
        if (rc) return rc;
        HD_HIP(fetch);
    }
    for (uint32_t s = 0; s < a->S; ++s) a->stream[s].decided_more(a->gate.p[s].n);
    return HD_OK;
}

// Its own: a stream without a modem is passed by, in front of the max_push test.  `cap`, the longest part of a row in the launch, sizes its LDS; behind
// the wait the host's copy of n and g follows the device's.  Then the scan.
int afsk_launch(hd_afsk* a, uint32_t max_n)
{
    if (const int rc = check_max_push(a, "hd_afsk", &max_n, [a](uint32_t s) { if (!a->stream[s].s.F) a->src.p[s].n_total = 0; })) return rc;
    uint32_t cap = 0;
    const int rc = launch_chunks(
        a, max_n, HD_AFSK_CHUNK, "afsk: the launch's chunk does not fit the LDS",
        [&](uint32_t, const hd::ClockedSrc& d) { cap = std::max(cap, d.n); },
        [&] {
            const uint32_t longest = cap;
            cap = 0;
            return hd::launch_afsk_slots(a->e->qa, a->S, longest, a->src.dev, a->st.p, a->ring32.base(), a->ring32.stride, a->ctab.p, a->slots.base(), a->slots.stride);
        },
        [&] {
            for (uint32_t s = 0; s < a->S; ++s) {
                hd::AfskState& m = a->stream[s].s;
                if (!m.F || !a->src.p[s].n) continue;
                m.n += a->src.p[s].n;
                m.g = hd::afsk_slots_before(m.F, m.n);
            }
        });
    if (rc) return rc;
    return afsk_scan(a);
}

// (The rings need no clearing: nothing in front of a stream's index 0 is read, and no candidate reads a slot that was not written since.)
int afsk_clear(hd_afsk* a, uint32_t s0, uint32_t ns)
{
    hipStream_t q = a->e->qa;
    for (uint32_t s = s0; s < s0 + ns; ++s) {
        a->stream[s].reset();
        HD_HIP(hipMemcpyAsync(a->st.p + s, &a->stream[s].s, sizeof(hd::AfskState), hipMemcpyHostToDevice, q));
    }
    HD_HIP(hipStreamSynchronize(q));
    return HD_OK;
}

}  // namespace

extern "C" {

void hd_afsk_params_default(hd_afsk_params* p) { if (p) hd::afsk_params_default(p); }

int hd_afsk_create(hd_engine* e, const hd_afsk_params* params, hd_afsk** out)
{
    if (!e || !out) return fail(HD_ERR_INVALID, "null argument");
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(e->mtx);
    std::unique_ptr<hd_afsk> a(new hd_afsk);
    a->e = e; a->S = e->S;
    hd::afsk_params_default(&a->prm);
    if (params) a->prm = *params;
    // (a launch takes at least one candidate of every active stream and its results must fit HD_AFSK_LAUNCH records)
    if (e->S > HD_AFSK_LAUNCH) return fail(HD_ERR_UNSUPPORTED, "hd_afsk_create: at most " + std::to_string(HD_AFSK_LAUNCH) + " streams");
    hd::AfskPatterns pat;
    const int ok = hd::afsk_params_check(a->prm, std::max<uint32_t>(e->n2_cap, 4096u), pat);
    if (ok == HD_ERR_INVALID)
        return fail(ok, "afsk parameters: 17 <= max_frame_bytes <= 332, repair_flips <= 4, at most 64 flip patterns with the untouched one");
    if (ok) return fail(ok, "afsk parameters: the slot ring holds 8 L + 72 + max_push <= " + std::to_string(HD_AFSK_RING) + " slots");
    if (const int rc = enter(e)) return rc;
    const uint32_t S = a->S;
    a->stream.resize(S);
    for (auto& st : a->stream) { st.pat = pat; st.require_addr = a->prm.require_addr; }
    a->h_count.resize(S);
    a->h_out.resize(HD_AFSK_LAUNCH);
    int32_t C[1024];
    hd::tones_table(C);
    HD_HIP(a->st.alloc_unfilled(S));
    HD_HIP(a->ring32.alloc((size_t)S * 4, hd::kAfskRing32, hd::kAfskGuard, hd::kAfskGuardWord, e->qa));
    HD_HIP(a->slots.alloc(S, HD_AFSK_RING, hd::kAfskGuard, hd::kAfskGuardWord, e->qa));
    HD_HIP(a->count.alloc(1, S, hd::kAfskGuard, hd::kAfskGuardWord, e->qa));
    HD_HIP(a->list.alloc(S, hd_afsk::kListCap, hd::kAfskGuard, hd::kAfskGuardWord, e->qa));
    HD_HIP(a->out.alloc(1, (size_t)HD_AFSK_LAUNCH * kAfskOutWords, hd::kAfskGuard, hd::kAfskGuardWord, e->qa));
    HD_HIP(a->pat.alloc_unfilled(1));
    HD_HIP(a->ctab.alloc_unfilled(1024));
    HD_HIP(a->src.alloc(S));
    HD_HIP(a->gate.alloc(S));
    HD_HIP(a->cand.alloc(S));
    HD_HIP(hipMemcpyAsync(a->ctab.p, C, sizeof C, hipMemcpyHostToDevice, e->qa));
    HD_HIP(hipMemcpyAsync(a->pat.p, &pat, sizeof pat, hipMemcpyHostToDevice, e->qa));
    if (const int rc = afsk_clear(a.get(), 0, S)) return rc;           // (waits for the queue: `C` and `pat` are locals)
    *out = a.release();
    return HD_OK;
}

void hd_afsk_destroy(hd_afsk* a) { destroy(a); }

int hd_afsk_reset(hd_afsk* a, uint32_t stream) { return reset(a, stream, afsk_clear); }

int hd_afsk_set_modem(hd_afsk* a, uint32_t stream, double baud, double mark_hz, double space_hz)
{
    if (const int rc = check_object(a, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(a->e->mtx);
    hd::AfskState m;
    const int rc = hd::afsk_modem(m, a->e->fsd, baud, mark_hz, space_hz);
    if (rc == HD_ERR_UNSUPPORTED) return fail(rc, "afsk: 8 <= decimated rate / baud <= " + std::to_string(HD_AFSK_MAX_SPB));
    if (rc) return fail(rc, "afsk: 0 < mark, space < decimated rate / 2, and two different tones");
    if (const int rc2 = enter(a->e)) return rc2;
    a->stream[stream].s = m;
    return afsk_clear(a, stream, 1);
}

int hd_afsk_set_bell202(hd_afsk* a, uint32_t stream) { return hd_afsk_set_modem(a, stream, 1200.0, 1200.0, 2200.0); }

int hd_afsk_push_engine(hd_afsk* a) { return push_engine(a, "hd_afsk_push_engine", afsk_launch); }

int hd_afsk_push_device(hd_afsk* a, const float* d_rows, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(a, d_rows, stride, n_per_stream, n, true, afsk_launch);
}

int hd_afsk_push_host(hd_afsk* a, const float* rows, size_t stride, const uint32_t* n_per_stream, uint32_t n)
{
    return push_rows(a, rows, stride, n_per_stream, n, false, afsk_launch);
}

int hd_afsk_take_frames(hd_afsk* a, uint32_t stream, hd_afsk_rx* out, size_t cap)
{
    if (const int rc = check_object(a, stream)) return rc;
    std::lock_guard<std::recursive_mutex> lock(a->e->mtx);
    if (const int rc = enter(a->e)) return rc;
    return (int)a->stream[stream].take(out, cap);
}

// (samples and slots are the device's own: a host copy that had drifted would show here)
int hd_afsk_stats(hd_afsk* a, uint32_t stream, hd_afsk_counters* out)
{
    if (const int rc = check_object(a, stream)) return rc;
    if (!out) return fail(HD_ERR_INVALID, "null output");
    std::lock_guard<std::recursive_mutex> lock(a->e->mtx);
    if (const int rc = enter(a->e)) return rc;
    hd::AfskState h;
    HD_HIP(hipMemcpy(&h, a->st.p + stream, sizeof h, hipMemcpyDeviceToHost));
    a->stream[stream].stats(out, h.n, h.g);
    return HD_OK;
}

// The measurement hook (tools/micro/afsk_rate.py; not part of the ABI): hd_afsk_push_engine with the slot launches and the gate and frame launches of its
// scan each between two HIP events (0 where none was launched), and the host time of the whole call in microseconds.
int hd_debug_afsk_push_timed(hd_afsk* a, float* slots_ms, float* scan_ms, double* host_us)
{
    if (!a || !slots_ms || !scan_ms || !host_us) return fail(HD_ERR_INVALID, "null argument");
    std::lock_guard<std::recursive_mutex> lock(a->e->mtx);
    if (const int rc = enter(a->e)) return rc;
    HD_HIP(hipEventCreate(&a->f0));
    HD_HIP(hipEventCreate(&a->f1));
    a->frames_launched = false;
    const int rc = push_timed(a, slots_ms, host_us, hd_afsk_push_engine);
    *scan_ms = 0;
    if (rc == HD_OK && a->frames_launched && hipEventQuery(a->f1) == hipSuccess) (void)hipEventElapsedTime(scan_ms, a->f0, a->f1);
    (void)hipGetLastError();
    (void)hipEventDestroy(a->f0); (void)hipEventDestroy(a->f1);
    a->f0 = a->f1 = nullptr;
    return rc;
}

// Test hooks (tests/test_gpu_afsk.py; not part of the ABI).  The records of the slots first .. first + n - 1 as the stream's ring holds them, n words.
int hd_debug_afsk_slots(hd_afsk* a, uint32_t stream, uint64_t first, int32_t* out, size_t n)
{
    if (!a || stream >= a->S || !out || n > HD_AFSK_RING) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(a->e->mtx);
    if (const int rc = enter(a->e)) return rc;
    for (size_t k = 0; k < n;) {
        const size_t at = (size_t)((first + k) & (HD_AFSK_RING - 1u)), run = std::min<size_t>(n - k, HD_AFSK_RING - at);
        HD_HIP(hipMemcpy(out + k, a->slots.row(stream) + at, run * sizeof(int32_t), hipMemcpyDeviceToHost));
        k += run;
    }
    return (int)n;
}

// The log of the stream's candidates, as hd_host_afsk_candidates.
int hd_debug_afsk_candidates(hd_afsk* a, uint32_t stream, hd_afsk_candidate* out, size_t cap)
{
    if (!a || stream >= a->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(a->e->mtx);
    if (const int rc = enter(a->e)) return rc;
    return (int)a->stream[stream].take_log(out, cap);
}

// The dynamic LDS a slot launch whose longest row has `cap` samples asks for, in bytes; 0: no such launch (tests/test_afsk_kernels.py holds the chunk's
// figure to two workgroups a CU).  No GPU is touched.
uint32_t hd_debug_afsk_slot_lds(uint32_t cap) { return hd::afsk_slots_lds_bytes(cap); }

// How many of the guard words around the stream's four rings, its slots and its list, the counts and the results no longer hold their pattern.
int hd_debug_afsk_guards(hd_afsk* a, uint32_t stream)
{
    if (!a || stream >= a->S) return fail(HD_ERR_INVALID, "bad argument");
    std::lock_guard<std::recursive_mutex> lock(a->e->mtx);
    if (const int rc = enter(a->e)) return rc;
    const size_t r = (size_t)stream * 4;
    return damaged_guards({{a->ring32, r}, {a->ring32, r + 1}, {a->ring32, r + 2}, {a->ring32, r + 3}, {a->slots, stream}, {a->list, stream}, {a->count, 0}, {a->out, 0}});
}

}  // extern "C"
