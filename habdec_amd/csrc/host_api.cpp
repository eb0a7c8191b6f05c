// C ABI over the host-side routines of the engine (include/habdec_amd_host.h).  No HIP calls in here.
#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/habdec_amd_host.h"
#include "host/afc_tracker.hpp"
#include "host/baud_probe.hpp"
#include "host/afsk.hpp"
#include "host/clocked.hpp"
#include "host/combine.hpp"
#include "host/fsk4.hpp"
#include "host/fsk4_track.hpp"
#include "host/ssdv.hpp"
#include "host/tones.hpp"
#include "host/tone_search.hpp"
#include "host/decim_plan.hpp"
#include "host/fir_design.hpp"
#include "host/fir_lds.hpp"
#include "host/format_trial.hpp"
#include "host/gui_payload.hpp"
#include "host/telemetry.hpp"
#include "host/sondehub.hpp"
#include "host/text_stage.hpp"
#include "host/iq_file_batch.hpp"
#include "host/survey.hpp"
#include "host/tune_host.hpp"
#include "host/waterfall.hpp"
#include "kernels/exact_math.h"

struct hd_host_rtty { hd::RttyFramer f; };
struct hd_host_text { hd::TextStage t; };
struct hd_host_afc { hd::AfcTracker a; };

static void put(char* dst, size_t cap, const std::string& s)
{
    if (!dst || !cap) return;
    const size_t n = std::min(cap - 1, s.size());
    std::memcpy(dst, s.data(), n);
    dst[n] = 0;
}

extern "C" {

int hd_host_decim_plan(unsigned total, int ratio[2], unsigned ntaps[2])
{
    std::vector<hd::DecimStage> st;
    if (!hd::decim_plan(total, st)) return -1;
    for (size_t i = 0; i < st.size(); ++i) { ratio[i] = st[i].ratio; ntaps[i] = (unsigned)st[i].taps.size(); }
    return (int)st.size();
}
size_t hd_host_decim_taps(unsigned total, int stage, float* taps, size_t cap)
{
    std::vector<hd::DecimStage> st;
    if (!hd::decim_plan(total, st) || stage < 0 || (size_t)stage >= st.size()) return 0;
    const auto& t = st[stage].taps;
    std::memcpy(taps, t.data(), std::min(cap, t.size()) * sizeof(float));
    return t.size();
}
size_t hd_host_lowpass_design(float cutoff_rel, float transition, size_t batch, size_t prev_ntaps, int float_trig, float* taps, size_t cap)
{
    hd::LowpassDesigner d;
    d.float_trig = float_trig != 0;
    d.batch = batch;
    d.taps.assign(prev_ntaps, 0.0f);
    if (!d.design(cutoff_rel, transition)) return 0;
    std::memcpy(taps, d.taps.data(), std::min(cap, d.taps.size()) * sizeof(float));
    return d.taps.size();
}
size_t hd_host_fir_demod_lds_bytes(uint32_t taps, size_t* static_bytes)
{
    if (static_bytes) *static_bytes = hd::kFirStaticLds;
    return hd::fir_demod_lds_bytes(taps);
}
uint32_t hd_host_fir_demod_max_taps(size_t lds_bytes) { return hd::fir_demod_max_taps(lds_bytes); }

hd_host_rtty* hd_host_rtty_new(size_t nbits, float nstops) { auto* r = new hd_host_rtty; r->f.nbits = nbits; r->f.nstops = nstops; return r; }
void hd_host_rtty_free(hd_host_rtty* r) { delete r; }
size_t hd_host_rtty_pending(const hd_host_rtty* r) { return r ? r->f.pending() : 0; }
size_t hd_host_rtty_push_run(hd_host_rtty* r, const uint8_t* bits, size_t n, char* out, size_t cap)
{
    r->f.push_bits(bits, n);
    std::string s;
    r->f.frame(s);
    std::memcpy(out, s.data(), std::min(cap, s.size()));
    return s.size();
}

void hd_host_crc16(const char* s, size_t n, char out4[5])
{
    const std::string r = hd::crc16_ccitt_hex(std::string(s, n));
    std::memcpy(out4, r.c_str(), 5);
}
int hd_host_extract_sentence(const char* stream, size_t n, char* callsign, char* data, char* crc, char* rest, size_t cap)
{
    hd::SentenceMatch m;
    if (!hd::extract_sentence(std::string(stream, n), m)) return 0;
    put(callsign, cap, m.callsign); put(data, cap, m.data); put(crc, cap, m.crc); put(rest, cap, m.rest);
    return 1;
}

hd_host_text* hd_host_text_new(size_t nbits, float nstops) { auto* t = new hd_host_text; t->t.framer.nbits = nbits; t->t.framer.nstops = nstops; return t; }
void hd_host_text_free(hd_host_text* t) { delete t; }
void hd_host_text_push_bits(hd_host_text* t, const uint8_t* bits, size_t n)
{
    if (n) t->t.framer.push_bits(bits, n);
    t->t.run(n != 0, [](const hd::SentenceMatch&) {});
}
size_t hd_host_text_get(hd_host_text* t, int which, char* buf, size_t cap)
{
    const std::string* s = &t->t.stream;
    if (which == 1) s = &t->t.last_sentence; else if (which == 2) s = &t->t.ok_log; else if (which == 3) s = &t->t.match_log; else if (which == 4) s = &t->t.char_log;
    put(buf, cap, *s);
    return s->size();
}

hd_host_afc* hd_host_afc_new(void) { return new hd_host_afc; }
void hd_host_afc_free(hd_host_afc* a) { delete a; }
void hd_host_afc_step(hd_host_afc* a, int have, int valid, int p1, int p2, float pw1, float pw2, double mean, double sigma, size_t bins, double rate)
{
    hd::SpectrumStats st{};
    st.valid = valid; st.peak1 = p1; st.peak2 = p2; st.power1 = pw1; st.power2 = pw2; st.mean = mean; st.sigma = sigma;
    a->a.step(have != 0, st, bins, rate);
}
void hd_host_afc_reset(hd_host_afc* a, double c, size_t bins, double rate) { a->a.reset(c, bins, rate); }
void hd_host_afc_get(hd_host_afc* a, double* c, double* sh, double* nf, double* ns, int* pl, int* pr)
{
    *c = a->a.correction; *sh = a->a.shift_hz; *nf = a->a.noise_floor; *ns = a->a.noise_sigma; *pl = a->a.gui_left; *pr = a->a.gui_right;
}

void hd_host_atan2f(const float* y, const float* x, float* out, size_t n) { for (size_t i = 0; i < n; ++i) out[i] = hd::exact_atan2f(y[i], x[i]); }
void hd_host_discriminate(const float* iq, size_t n, float pr, float pi, float* out)
{
    for (size_t i = 0; i < n; ++i) { out[i] = hd::discriminate(iq[2 * i], iq[2 * i + 1], pr, pi); pr = iq[2 * i]; pi = iq[2 * i + 1]; }
}

/* ---- GUI payloads (habdec_ws_protocol.cpp:338-429, NetTransport.h, CompressedVector.cpp; see host/gui_payload.hpp) ---- */
size_t hd_host_spectrum_payload(const float* bins, size_t n, double noise_floor, double noise_variance, double sampling_rate, double shift,
                                int peak_left, int peak_right, float zoom, int resolution, int type_size, uint8_t* out, size_t cap,
                                size_t* bins_sent)
{
    if (bins_sent) *bins_sent = 0;
    if (!bins && n) return 0;
    hd::gui::SpectrumMeta m;
    m.noise_floor = noise_floor; m.noise_variance = noise_variance; m.sampling_rate = sampling_rate; m.shift = shift;
    // Decoder::getSpectrumInfo (Decoder.h:823-828): the sign of a peak carries its validity
    m.peak_left = peak_left < 0 ? -peak_left : peak_left; m.peak_left_valid = peak_left > 0;
    m.peak_right = peak_right < 0 ? -peak_right : peak_right; m.peak_right_valid = peak_right > 0;
    std::vector<uint8_t> o;
    const size_t sent = hd::gui::spectrum_payload(std::vector<float>(bins, bins + n), m, zoom, resolution, type_size, o);
    if (bins_sent) *bins_sent = sent;
    if (out && cap >= o.size()) std::memcpy(out, o.data(), o.size());
    return o.size();
}
size_t hd_host_demod_payload(const float* trace, size_t n, int resolution, int type_size, uint8_t* out, size_t cap, size_t* sent_out)
{
    if (sent_out) *sent_out = 0;
    if (!trace && n) return 0;
    std::vector<uint8_t> o;
    const size_t sent = hd::gui::demod_payload(std::vector<float>(trace, trace + n), resolution, type_size, o);
    if (sent_out) *sent_out = sent;
    if (out && cap >= o.size()) std::memcpy(out, o.data(), o.size());
    return o.size();
}

/* ---- post-decode telemetry (sentence_parse.cpp, GpsDistance.cpp; see host/telemetry.hpp) ---- */
int hd_host_parse_time(const char* text, int* hour, int* minute, float* second)
{
    if (!text || !hour || !minute || !second) return -1;
    return (int)hd::telemetry::parse_time(text, *hour, *minute, *second);
}
int hd_host_parse_gps_pos(const char* text, float* out)
{
    if (!text || !out) return -1;
    return (int)hd::telemetry::parse_gps_pos(text, *out);
}
int hd_host_parse_sentence(const char* sentence_without_crc, hd_host_telemetry* out)
{
    if (!sentence_without_crc || !out) return -1;
    hd::telemetry::Fields f;
    const auto st = hd::telemetry::parse_sentence(sentence_without_crc, f);
    if (st != hd::telemetry::Status::Ok) return (int)st;
    std::memset(out, 0, sizeof *out);
    std::strncpy(out->callsign, f.callsign.c_str(), sizeof out->callsign - 1);
    out->frame = f.frame; out->hour = f.hour; out->minute = f.minute; out->second = f.second;
    out->lat = f.lat; out->lon = f.lon; out->alt = f.alt;
    return 1;
}
size_t hd_host_timestamp_from_hms(int64_t now_unix, int hour, int minute, float second, char* buf, size_t cap)
{
    const std::string s = hd::telemetry::timestamp_from_hms(now_unix, hour, minute, second);
    if (buf && cap) { const size_t n = std::min(cap - 1, s.size()); std::memcpy(buf, s.data(), n); buf[n] = 0; }
    return s.size();
}
void hd_host_gps_distance(double lat1, double lon1, double alt1, double lat2, double lon2, double alt2, double out[5])
{
    const auto d = hd::telemetry::gps_distance(lat1, lon1, alt1, lat2, lon2, alt2);
    out[0] = d.line; out[1] = d.circle; out[2] = d.radians; out[3] = d.elevation_deg; out[4] = d.bearing_deg;
}

/* ---- sondehub upload batch (sondehub_uploader.cpp:14-69, main.cpp:286-306; see host/sondehub.hpp) ---- */
struct hd_host_sondehub {
    hd::SondehubBatch b;
    std::string pending;      // a body that did not fit the caller's buffer: handed out again by the next take
    size_t pending_n = 0;
    hd_host_sondehub(const char* u, const char* v) : b(u ? u : "", v ? v : "") {}
};
hd_host_sondehub* hd_host_sondehub_new(const char* uploader_callsign, const char* software_version) { return new hd_host_sondehub(uploader_callsign, software_version); }
void hd_host_sondehub_free(hd_host_sondehub* h) { delete h; }
int hd_host_sondehub_push_sentence(hd_host_sondehub* h, uint32_t stream, const char* callsign, const char* data, int64_t now_unix_ns)
{
    if (!h || !callsign || !data) return -1;
    return h->b.push_sentence(stream, callsign, data, now_unix_ns);
}
int hd_host_sondehub_push(hd_host_sondehub* h, const char* payload_callsign, const char* time_received, const char* datetime, int frame, float lat, float lon, float alt)
{
    if (!h || !payload_callsign || !time_received || !datetime) return -1;
    hd::SondeRecord r;
    r.payload_callsign = payload_callsign; r.time_received = time_received; r.datetime = datetime; r.frame = frame; r.lat = lat; r.lon = lon; r.alt = alt;
    h->b.push(r);
    return 1;
}
size_t hd_host_sondehub_size(const hd_host_sondehub* h) { return h ? h->b.size() : 0; }
size_t hd_host_sondehub_take(hd_host_sondehub* h, int64_t now_unix_ns, char* out, size_t cap, size_t* n_records)
{
    if (!h) return 0;
    if (h->pending.empty()) h->pending = h->b.take(now_unix_ns, &h->pending_n);
    const size_t n = h->pending.size();
    if (n_records) *n_records = h->pending_n;
    if (out && cap > n) { std::memcpy(out, h->pending.data(), n); out[n] = 0; h->pending.clear(); h->pending_n = 0; }
    return n;
}
size_t hd_host_utc_iso(int64_t unix_ns, char* buf, size_t cap)
{
    const std::string s = hd::utc_iso_ns(unix_ns);
    if (buf && cap) { const size_t n = std::min(cap - 1, s.size()); std::memcpy(buf, s.data(), n); buf[n] = 0; }
    return s.size();
}
size_t hd_host_json_number(double v, char* buf, size_t cap)
{
    const std::string s = hd::json_number(v);
    if (buf && cap) { const size_t n = std::min(cap - 1, s.size()); std::memcpy(buf, s.data(), n); buf[n] = 0; }
    return s.size();
}

/* ---- batched cf32 file ingest (IQSource_File.h:124-172 per file; see host/iq_file_batch.hpp) ---- */
hd_host_iqfiles* hd_host_iqfiles_open(const char* const* paths, uint32_t n_files, int loop, uint32_t chunk, uint32_t granule, double realtime_rate)
{
    return hd_host_iqfiles_open_fmt(paths, n_files, loop, chunk, granule, realtime_rate, HD_IQ_CF32);
}
hd_host_iqfiles* hd_host_iqfiles_open_fmt(const char* const* paths, uint32_t n_files, int loop, uint32_t chunk, uint32_t granule, double realtime_rate, int fmt)
{
    if (!paths || !n_files || !hd::iq_bytes(fmt)) return nullptr;
    std::vector<std::string> v;
    for (uint32_t i = 0; i < n_files; ++i) { if (!paths[i]) return nullptr; v.emplace_back(paths[i]); }
    auto* h = new hd_host_iqfiles;
    if (!h->batch.open(v, loop != 0, chunk, granule, realtime_rate, fmt)) { delete h; return nullptr; }
    return h;
}
void hd_host_iqfiles_close(hd_host_iqfiles* h) { delete h; }
uint32_t hd_host_iqfiles_streams(const hd_host_iqfiles* h) { return h ? h->batch.streams() : 0; }
uint64_t hd_host_iqfiles_count(const hd_host_iqfiles* h, uint32_t stream) { return (h && stream < h->batch.streams()) ? h->batch.file(stream).count() : 0; }
uint64_t hd_host_iqfiles_rewinds(const hd_host_iqfiles* h, uint32_t stream) { return (h && stream < h->batch.streams()) ? h->batch.file(stream).rewinds() : 0; }
uint32_t hd_host_iqfiles_next(hd_host_iqfiles* h, float* slab, size_t stride, uint32_t* n_per_stream)
{
    if (!h || !slab || !n_per_stream || stride < h->batch.chunk()) return 0;
    return h->batch.next(slab, stride, n_per_stream);
}
uint32_t hd_host_iqfiles_next_raw(hd_host_iqfiles* h, void* slab, size_t stride, uint32_t* n_per_stream)
{
    if (!h || !slab || !n_per_stream || stride < h->batch.chunk()) return 0;
    return h->batch.next_raw(slab, stride, n_per_stream);
}
size_t hd_host_iq_bytes(int fmt) { return hd::iq_bytes(fmt); }
void hd_host_iq_convert(int fmt, const void* src, size_t n, float* out) { if (src && out) hd::iq_convert(fmt, src, n, out); }

/* ---- per-stream tuning (kernels/tune.h) ---- */
int hd_host_tune_step(double offset_hz, double decimated_rate, uint32_t* step)
{
    uint32_t d = 0;
    if (!hd::tune_step(offset_hz, decimated_rate, &d)) return -1;     // HD_ERR_INVALID
    if (step) *step = d;
    return 0;
}
void hd_host_tune_tables(float coarse[512], float fine[512]) { hd::tune_tables(coarse, fine); }
void hd_host_tune_rotate(const float* iq, size_t n, uint32_t phase, uint32_t step, float* out)
{
    float tab[4 * hd::kTuneTable];
    hd::tune_tables(tab, tab + 2 * hd::kTuneTable);
    hd::tune_rotate(tab, iq, n, phase, step, out);
}

/* ---- wideband survey (kernels/survey.hip; see host/survey.hpp) ---- */
void hd_host_survey_window(float w[4096]) { if (w) hd::survey_window(w); }
int hd_host_survey_detect(const double* power, uint64_t segments, double sampling_rate, const hd_survey_params* p, hd_survey_candidate* out, uint32_t cap,
                          uint32_t* found)
{
    return hd::survey_detect(power, segments, sampling_rate, p, out, cap, found);
}

/* ---- waterfall (kernels/waterfall.hip; see host/waterfall.hpp) ---- */
void hd_host_waterfall_params_default(hd_waterfall_params* p) { if (p) hd::waterfall_params_default(p); }
int hd_host_waterfall_detect_row(const float* row, uint32_t segments, double sampling_rate, const hd_waterfall_params* p, hd_waterfall_row* hdr,
                                 uint32_t* marks)
{
    return hd::waterfall_detect_row(row, segments, sampling_rate, p, hdr, marks);
}
int hd_host_waterfall_tracks(const hd_waterfall_row* headers, const uint32_t* marks, uint64_t n_rows, double sampling_rate,
                             const hd_waterfall_track_params* p, hd_waterfall_track* out, uint32_t cap, uint32_t* found)
{
    return hd::waterfall_tracks(headers, marks, n_rows, sampling_rate, p, out, cap, found);
}

/* ---- clocked decoder (kernels/clocked.hip; see host/clocked.hpp, host/chase_repair.hpp) ---- */
struct hd_host_clocked {
    double fsd;
    hd::ClockedStream st;
    hd::ClockedText tx;
    hd_host_clocked(double rate, uint32_t cap) : fsd(rate), st(cap) {}
    void drain(hd_clocked_record* out, size_t cap, size_t* n)
    {
        std::vector<hd_clocked_record> tmp(out ? std::min<size_t>(cap, st.take(nullptr, 0)) : st.take(nullptr, 0));
        const size_t k = st.take(tmp.data(), tmp.size());
        tx.feed(tmp.data(), k);
        if (out && k) std::memcpy(out, tmp.data(), k * sizeof(hd_clocked_record));
        *n = k;
    }
};
hd_host_clocked* hd_host_clocked_new(double decimated_rate, const hd_clocked_params* params)
{
    hd_clocked_params prm;
    hd::clocked_params_default(&prm);
    if (params) prm = *params;
    if (!hd::clocked_params_ok(&prm) || !(decimated_rate > 0)) return nullptr;
    auto* h = new hd_host_clocked(decimated_rate, prm.record_cap);
    h->tx.repair_bits = prm.repair_bits; h->tx.repair_flips = prm.repair_flips;
    return h;
}
void hd_host_clocked_free(hd_host_clocked* h) { delete h; }
void hd_host_clocked_reset(hd_host_clocked* h) { if (h) { h->st.reset(); h->tx.reset(); } }
int hd_host_clocked_set_modem(hd_host_clocked* h, double baud, uint32_t nbits, uint32_t nstops, int invert)
{
    if (!h) return HD_ERR_INVALID;
    const uint32_t F = hd::clocked_modem_F(h->fsd, baud, nbits, (double)nstops);
    if (!F) return HD_ERR_UNSUPPORTED;
    h->st.set_modem(F, nbits, nstops, invert ? 1u : 0u);
    h->tx.reset(); h->tx.nbits = nbits;
    return HD_OK;
}
void hd_host_clocked_push(hd_host_clocked* h, const float* d, size_t n) { if (h && d && n) h->st.push(d, n); }
int hd_host_clocked_records(hd_host_clocked* h, hd_clocked_record* out, size_t cap)
{
    if (!h) return HD_ERR_INVALID;
    if (!out) return (int)h->st.take(nullptr, 0);
    size_t n = 0;
    h->drain(out, cap, &n);
    return (int)n;
}
int hd_host_clocked_take_sentences(hd_host_clocked* h, hd_clocked_sentence* out, size_t cap)
{
    if (!h || (cap && !out)) return HD_ERR_INVALID;
    size_t n = 0;
    h->drain(nullptr, 0, &n);
    return (int)h->tx.take(out, cap);
}
int hd_host_clocked_stats(const hd_host_clocked* h, hd_clocked_counters* out)
{
    if (!h || !out) return HD_ERR_INVALID;
    const hd::ClockedState& s = h->st.s;
    *out = hd_clocked_counters{s.n, s.p, s.chars, s.rejects, s.dropped, h->tx.matches_failed, h->tx.plain, h->tx.repaired};
    return HD_OK;
}
int hd_host_chase_repair(const char* span, size_t n, const int32_t* data, uint32_t nbits, uint32_t repair_bits, uint32_t repair_flips, char* out,
                         uint32_t* flips)
{
    if (!span || !data || !out || !flips || (nbits != 7 && nbits != 8) || repair_bits > hd::kChaseMaxBits || repair_flips > hd::kChaseMaxFlips) return HD_ERR_INVALID;
    std::string fixed;
    hd::SentenceMatch m;
    *flips = hd::chase_repair(std::string(span, n), data, nbits, repair_bits, repair_flips, fixed, m);
    if (!*flips) return 0;
    std::memcpy(out, fixed.data(), n);
    return 1;
}

/* ---- tone-filter demodulator (kernels/tones.hip; see host/tones.hpp) ---- */
struct hd_host_tones {
    double fsd;
    uint32_t window_q8;
    hd::TonesStream st;
};
hd_host_tones* hd_host_tones_new(double decimated_rate, const hd_tones_params* params)
{
    hd_tones_params prm;
    hd::tones_params_default(&prm);
    if (params) prm = *params;
    if (!(decimated_rate > 0)) return nullptr;
    auto* h = new hd_host_tones;
    h->fsd = decimated_rate; h->window_q8 = prm.window_q8;
    return h;
}
void hd_host_tones_free(hd_host_tones* h) { delete h; }
void hd_host_tones_reset(hd_host_tones* h) { if (h) h->st.reset(); }
int hd_host_tones_set_modem(hd_host_tones* h, double baud, double f_hi_hz, double f_lo_hz)
{
    if (!h) return HD_ERR_INVALID;
    return hd::tones_modem(h->st.s, h->fsd, baud, f_hi_hz, f_lo_hz, h->window_q8);
}
size_t hd_host_tones_push(hd_host_tones* h, const float* iq, size_t n, float* out) { return h && iq && out && n ? h->st.push(iq, n, out) : 0; }
int hd_host_tones_stats(const hd_host_tones* h, hd_tones_info* out)
{
    if (!h || !out) return HD_ERR_INVALID;
    const hd::TonesState& s = h->st.s;
    *out = hd_tones_info{s.n, s.F, s.full, s.W, s.L, s.phi[0], s.phi[1]};
    return HD_OK;
}

/* ---- tone search (kernels/tone_search.hip; see host/tone_search.hpp) ---- */
struct hd_host_tone_search {
    hd::ToneSearchStream st;
};
int hd_host_tone_search_detect(const double* p, uint64_t segments, double fsd, const hd_tone_search_detect_params* params, hd_tone_search_result* out)
{
    return hd::tone_search_detect(p, segments, fsd, params, out);
}
hd_host_tone_search* hd_host_tone_search_create(void) { return new hd_host_tone_search; }
void hd_host_tone_search_destroy(hd_host_tone_search* h) { delete h; }
void hd_host_tone_search_reset(hd_host_tone_search* h) { if (h) h->st.reset(); }
void hd_host_tone_search_push(hd_host_tone_search* h, const float* iq, size_t n) { if (h && iq && n) h->st.push(iq, n); }
int hd_host_tone_search_power(const hd_host_tone_search* h, double* p, size_t cap, uint64_t* segments)
{
    if (!h || !p) return HD_ERR_INVALID;
    if (segments) *segments = h->st.segments;
    if (cap < hd::kToneSearchBins) return 0;
    h->st.power(p);
    return (int)hd::kToneSearchBins;
}

/* ---- diversity combiner (kernels/combine.hip; see host/combine.hpp) ---- */
struct hd_host_combine {
    hd::CombineHostGroup g;
};
hd_host_combine* hd_host_combine_create(const uint32_t* streams, uint32_t count)
{
    auto* h = new hd_host_combine;
    if (!h->g.make(streams, count)) { delete h; return nullptr; }
    return h;
}
void hd_host_combine_destroy(hd_host_combine* h) { delete h; }
void hd_host_combine_reset(hd_host_combine* h) { if (h) h->g.reset(); }
int hd_host_combine_set_delay(hd_host_combine* h, uint32_t m, uint32_t delay)
{
    if (!h || m >= h->g.count || delay > HD_COMBINE_MAX_DELAY) return HD_ERR_INVALID;
    h->g.delay[m] = delay;
    return HD_OK;
}
int hd_host_combine_set_weight(hd_host_combine* h, uint32_t m, uint32_t weight)
{
    if (!h || m >= h->g.count || weight > 256u) return HD_ERR_INVALID;
    h->g.weight[m] = weight;
    return HD_OK;
}
int hd_host_combine_push(hd_host_combine* h, const float* rows, size_t stride, const uint32_t* n_per_member, uint32_t n, float* out)
{
    if (!h) return HD_ERR_INVALID;
    const uint32_t len = n_per_member ? n_per_member[0] : n;
    for (uint32_t m = 1; n_per_member && m < h->g.count; ++m) if (n_per_member[m] != len) return HD_ERR_INVALID;
    if (!len) return HD_OK;
    if (!rows || !out || (h->g.count > 1 && len > stride)) return HD_ERR_INVALID;
    h->g.push(rows, stride, len, out);
    return HD_OK;
}
int hd_host_combine_lags(hd_host_combine* h, const hd_combine_lag_params* p, hd_combine_lag* out, size_t cap)
{
    if (!h || !p || !out || cap < h->g.count) return HD_ERR_INVALID;
    return h->g.lags(p, out);
}
int hd_host_combine_align(hd_host_combine* h, const hd_combine_lag_params* p, hd_combine_lag* out, size_t cap)
{
    if (const int rc = hd_host_combine_lags(h, p, out, cap)) return rc;
    return hd::combine_align(out, h->g.count, h->g.delay, h->g.weight);
}
int hd_host_combine_scores(const hd_host_combine* h, uint32_t m, int32_t* out, size_t cap)
{
    if (!h || m < 1 || m >= h->g.count) return HD_ERR_INVALID;
    if (h->g.scores.empty()) return 0;
    const size_t k = 2 * (size_t)h->g.scores_L + 1;
    if (out && cap >= k) std::memcpy(out, h->g.scores.data() + (size_t)(m - 1) * k, k * sizeof(int32_t));
    return (int)k;
}
int hd_host_combine_stats(const hd_host_combine* h, uint32_t m, hd_combine_info* out)
{
    if (!h || !out || m >= h->g.count) return HD_ERR_INVALID;
    *out = hd_combine_info{h->g.n, h->g.stream[0], h->g.delay[m], h->g.weight[m], h->g.count};
    return HD_OK;
}

/* ---- SSDV packets (kernels/ssdv.hip; see host/ssdv.hpp) ---- */
struct hd_host_ssdv {
    hd::SsdvStream s;
};
hd_host_ssdv* hd_host_ssdv_create(const hd_ssdv_params* params)
{
    hd_ssdv_params p;
    hd::ssdv_params_default(&p);
    if (params) p = *params;
    if (!hd::ssdv_params_ok(&p)) return nullptr;
    auto* h = new hd_host_ssdv;
    h->s.max_fill = p.max_fill;
    return h;
}
void hd_host_ssdv_destroy(hd_host_ssdv* h) { delete h; }
void hd_host_ssdv_reset(hd_host_ssdv* h) { if (h) h->s.reset(); }
int hd_host_ssdv_push_bytes(hd_host_ssdv* h, const uint8_t* bytes, const uint32_t* conf, size_t n)
{
    if (!h || (n && !bytes)) return HD_ERR_INVALID;
    h->s.push_bytes(bytes, conf, n);
    h->s.scan();
    return HD_OK;
}
int hd_host_ssdv_push_records(hd_host_ssdv* h, const hd_clocked_record* records, size_t n, uint32_t char_len)
{
    if (!h || (n && !records)) return HD_ERR_INVALID;
    h->s.push_records(records, n, char_len);
    h->s.scan();
    return HD_OK;
}
int hd_host_ssdv_take_packets(hd_host_ssdv* h, hd_ssdv_packet* out, size_t cap)
{
    if (!h) return HD_ERR_INVALID;
    return (int)h->s.take(out, cap);
}
int hd_host_ssdv_stats(const hd_host_ssdv* h, hd_ssdv_counters* out)
{
    if (!h || !out) return HD_ERR_INVALID;
    h->s.stats(out);
    return HD_OK;
}
void hd_host_ssdv_encode(const uint8_t* data223, uint8_t* parity32) { if (data223 && parity32) hd::ssdv_encode(data223, parity32); }
void hd_host_ssdv_make_packet(uint8_t type, const char* callsign, uint8_t image_id, uint16_t packet_id, uint16_t width, uint16_t height, uint8_t flags,
                              uint8_t mcu_offset, uint16_t mcu_index, const uint8_t* payload205, uint8_t* out256)
{
    if (payload205 && out256) hd::ssdv_make_packet(type, callsign, image_id, packet_id, width, height, flags, mcu_offset, mcu_index, payload205, out256);
}

/* ---- Horus Binary 4FSK (kernels/fsk4.hip; see host/fsk4.hpp) ---- */
struct hd_host_fsk4 {
    double fsd;
    hd_fsk4_params prm;
    hd::Fsk4Stream st;
};
int hd_fsk4_frame_preset(int preset, hd_fsk4_frame* out) { return out && hd::fsk4_preset(preset, out) ? HD_OK : out ? HD_ERR_UNSUPPORTED : HD_ERR_INVALID; }
hd_host_fsk4* hd_host_fsk4_new(double decimated_rate, const hd_fsk4_params* params)
{
    hd_fsk4_params prm;
    hd::fsk4_params_default(&prm);
    if (params) prm = *params;
    if (!(decimated_rate > 0) || !hd::fsk4_window_ok(prm.window_q8) || !hd::fsk4_params_ok(&prm)) return nullptr;
    if (!prm.max_push) prm.max_push = 4096;
    auto* h = new hd_host_fsk4;
    h->fsd = decimated_rate; h->prm = prm;
    h->st.set_params(prm);
    h->st.host_rings(prm.max_push);
    return h;
}
void hd_host_fsk4_free(hd_host_fsk4* h) { delete h; }
void hd_host_fsk4_reset(hd_host_fsk4* h) { if (h) h->st.reset(); }
int hd_host_fsk4_set_modem(hd_host_fsk4* h, double baud, double f0_hz, double spacing_hz, const hd_fsk4_frame* frame)
{
    if (!h || !frame) return HD_ERR_INVALID;
    hd::Fsk4Tab tab;
    if (!hd::fsk4_tables(*frame, tab)) return HD_ERR_UNSUPPORTED;
    hd::Fsk4State m;
    if (const int rc = hd::fsk4_modem(m, h->fsd, baud, f0_hz, spacing_hz, h->prm.window_q8)) return rc;
    h->st.s = m; h->st.tab = tab;
    h->st.reset();
    return HD_OK;
}
int hd_host_fsk4_retune(hd_host_fsk4* h, double f0_hz, double spacing_hz, uint64_t at_sample)
{
    if (!h || !h->st.s.F) return HD_ERR_INVALID;
    uint32_t phi[4];
    if (const int rc = hd::fsk4_retune_steps(h->fsd, f0_hz, spacing_hz, phi)) return rc;
    h->st.retune(phi, at_sample);
    h->st.apply_retunes();
    return HD_OK;
}
int hd_host_fsk4_retune_stats(const hd_host_fsk4* h, hd_fsk4_retune_info* out)
{
    if (!h || !out) return HD_ERR_INVALID;
    *out = hd_fsk4_retune_info{h->st.retunes, h->st.late, h->st.pending.size(), {h->st.s.psi[0], h->st.s.psi[1], h->st.s.psi[2], h->st.s.psi[3]}};
    return HD_OK;
}
// (in pieces of max_push, a scan behind each: the slot ring holds what one piece adds to the candidates that wait)
size_t hd_host_fsk4_push(hd_host_fsk4* h, const float* iq, size_t n)
{
    if (!h || !iq || !h->st.s.F) return 0;
    for (size_t at = 0; at < n;) {
        const size_t k = std::min<size_t>(n - at, h->prm.max_push);
        h->st.push_samples(iq + 2 * at, k);
        h->st.scan();
        at += k;
    }
    return n;
}
int hd_host_fsk4_take_frames(hd_host_fsk4* h, hd_fsk4_rx* out, size_t cap) { return h ? (int)h->st.take(out, cap) : HD_ERR_INVALID; }
int hd_host_fsk4_stats(const hd_host_fsk4* h, hd_fsk4_counters* out)
{
    if (!h || !out) return HD_ERR_INVALID;
    h->st.stats(out, h->st.s.n, h->st.s.g);
    return HD_OK;
}
size_t hd_host_fsk4_slots(const hd_host_fsk4* h, uint64_t first, uint32_t* out, size_t n)
{
    if (!h || !out || first + n > h->st.s.g || h->st.s.g - first > h->st.slot_cap) return 0;
    for (size_t k = 0; k < n; ++k) std::memcpy(out + 4 * k, &h->st.slots[(size_t)((first + k) & (h->st.slot_cap - 1u)) * 4u], 4 * sizeof(uint32_t));
    return n;
}
int hd_host_fsk4_candidates(hd_host_fsk4* h, hd_fsk4_candidate* out, size_t cap) { return h ? (int)h->st.take_log(out, cap) : HD_ERR_INVALID; }
size_t hd_host_fsk4_encode(const hd_fsk4_frame* frame, const uint8_t* payload, uint8_t* out) { return frame && payload && out ? hd::fsk4_encode(*frame, payload, out) : 0; }
uint32_t hd_host_fsk4_crc16(const uint8_t* bytes, size_t n) { return bytes || !n ? hd::fsk4_crc16(bytes, n) : 0xFFFFu; }

/* ---- 4FSK tone tracker (kernels/fsk4_track.hip; see host/fsk4_track.hpp) ---- */
int hd_host_fsk4_comb_detect(const double* acc, double decimated_rate, const hd_fsk4_comb_params* p, hd_fsk4_comb_record* out)
{
    if (out) std::memset(out, 0, sizeof *out);
    if (!acc || !p || !out) return HD_ERR_INVALID;
    hd::Fsk4CombPlan pl;
    if (const int rc = hd::fsk4_comb_plan(decimated_rate, p->baud, p->spacing_lo_hz, p->spacing_hi_hz, p->f_lo_hz, p->f_hi_hz, pl)) return rc;
    hd::fsk4_comb_detect(acc, pl, p->min_quality_q8, p->segments_ok != 0, out);
    return HD_OK;
}
struct hd_host_fsk4_track { hd::Fsk4TrackStream t; };
hd_host_fsk4_track* hd_host_fsk4_track_new(double decimated_rate, const hd_fsk4_track_params* params)
{
    hd_fsk4_track_params prm;
    hd::fsk4_track_params_default(&prm);
    if (params) prm = *params;
    if (!(decimated_rate > 0) || !hd::fsk4_track_params_ok(&prm)) return nullptr;
    auto* h = new hd_host_fsk4_track;
    h->t.prm = prm; h->t.fsd = decimated_rate;
    return h;
}
void hd_host_fsk4_track_free(hd_host_fsk4_track* h) { delete h; }
void hd_host_fsk4_track_reset(hd_host_fsk4_track* h) { if (h) h->t.reset(); }
int hd_host_fsk4_track_set_stream(hd_host_fsk4_track* h, double baud, double spacing_lo_hz, double spacing_hi_hz, double f_lo_hz, double f_hi_hz)
{
    if (!h) return HD_ERR_INVALID;
    hd::Fsk4CombPlan pl;
    if (const int rc = hd::fsk4_comb_plan(h->t.fsd, baud, spacing_lo_hz, spacing_hi_hz, f_lo_hz, f_hi_hz, pl)) return rc;
    h->t.book.plan = pl; h->t.book.baud = baud; h->t.book.set = true;
    h->t.reset();
    return HD_OK;
}
void hd_host_fsk4_track_attach(hd_host_fsk4_track* h, hd_host_fsk4* modem) { if (h) h->t.modem = modem ? &modem->st : nullptr; }
void hd_host_fsk4_track_push(hd_host_fsk4_track* h, const float* iq, size_t n) { if (h && iq && n) h->t.push(iq, n); }
int hd_host_fsk4_track_records(hd_host_fsk4_track* h, hd_fsk4_track_est* out, size_t cap) { return h ? (int)h->t.book.take_log(out, cap, true) : HD_ERR_INVALID; }
int hd_host_fsk4_track_stats(const hd_host_fsk4_track* h, hd_fsk4_track_info* out)
{
    if (!h || !out) return HD_ERR_INVALID;
    h->t.book.stats(out);
    return HD_OK;
}
int hd_host_fsk4_track_acc(const hd_host_fsk4_track* h, double* out)
{
    if (!h || !out) return HD_ERR_INVALID;
    std::memcpy(out, h->t.ts.acc.data(), hd::kFsk4CombBins * sizeof(double));
    return (int)hd::kFsk4CombBins;
}

/* ---- AFSK / AX.25 (kernels/afsk.hip; see host/afsk.hpp) ---- */
struct hd_host_afsk {
    double fsd;
    hd_afsk_params prm;
    hd::AfskStream st;
};
hd_host_afsk* hd_host_afsk_new(double decimated_rate, const hd_afsk_params* params)
{
    hd_afsk_params prm;
    hd::afsk_params_default(&prm);
    if (params) prm = *params;
    hd::AfskPatterns pat;
    if (!(decimated_rate > 0) || hd::afsk_params_check(prm, 4096u, pat)) return nullptr;
    auto* h = new hd_host_afsk;
    h->fsd = decimated_rate; h->prm = prm;
    h->st.pat = pat; h->st.require_addr = prm.require_addr;
    h->st.host_rings();
    return h;
}
void hd_host_afsk_free(hd_host_afsk* h) { delete h; }
void hd_host_afsk_reset(hd_host_afsk* h) { if (h) h->st.reset(); }
int hd_host_afsk_set_modem(hd_host_afsk* h, double baud, double mark_hz, double space_hz)
{
    if (!h) return HD_ERR_INVALID;
    hd::AfskState m;
    if (const int rc = hd::afsk_modem(m, h->fsd, baud, mark_hz, space_hz)) return rc;
    h->st.s = m;
    h->st.reset();
    return HD_OK;
}
// (in pieces of max_push, a scan behind each: the slot ring holds what one piece adds to the slots that wait)
size_t hd_host_afsk_push(hd_host_afsk* h, const float* row, size_t n)
{
    if (!h || !row || !h->st.s.F) return 0;
    for (size_t at = 0; at < n;) {
        const size_t k = std::min<size_t>(n - at, h->prm.max_push);
        h->st.push_samples(row + at, k);
        h->st.scan();
        at += k;
    }
    return n;
}
int hd_host_afsk_take_frames(hd_host_afsk* h, hd_afsk_rx* out, size_t cap) { return h ? (int)h->st.take(out, cap) : HD_ERR_INVALID; }
int hd_host_afsk_stats(const hd_host_afsk* h, hd_afsk_counters* out)
{
    if (!h || !out) return HD_ERR_INVALID;
    h->st.stats(out, h->st.s.n, h->st.s.g);
    return HD_OK;
}
size_t hd_host_afsk_slots(const hd_host_afsk* h, uint64_t first, int32_t* out, size_t n)
{
    if (!h || !out || first + n > h->st.s.g || h->st.s.g - first > HD_AFSK_RING) return 0;
    for (size_t k = 0; k < n; ++k) out[k] = h->st.slot_d(first + k);
    return n;
}
int hd_host_afsk_candidates(hd_host_afsk* h, hd_afsk_candidate* out, size_t cap) { return h ? (int)h->st.take_log(out, cap) : HD_ERR_INVALID; }
uint32_t hd_host_afsk_crc16(const uint8_t* bytes, size_t n) { return bytes || !n ? hd::afsk_crc16(bytes, n) : 0u; }
size_t hd_host_ax25_frame(const char* path, const uint8_t* info, size_t n_info, uint8_t* out, size_t cap)
{
    if (!path || (!info && n_info) || !out) return 0;
    const std::vector<uint8_t> f = hd::ax25_frame(path, info, n_info);
    if (f.empty() || f.size() > cap) return 0;
    std::memcpy(out, f.data(), f.size());
    return f.size();
}
size_t hd_host_ax25_levels(const uint8_t* frame, size_t n, uint32_t flags_before, uint32_t flags_after, uint8_t* out, size_t cap)
{
    if (!frame && n) return 0;
    const std::vector<uint8_t> lv = hd::ax25_levels(frame, n, flags_before, flags_after);
    if (out && lv.size() <= cap) std::memcpy(out, lv.data(), lv.size());
    return lv.size();
}
size_t hd_host_ax25_encode(const char* path, const uint8_t* info, size_t n_info, uint32_t flags_before, uint32_t flags_after, uint8_t* out, size_t cap)
{
    if (!path || (!info && n_info)) return 0;
    const std::vector<uint8_t> f = hd::ax25_frame(path, info, n_info);
    if (f.empty()) return 0;
    return hd_host_ax25_levels(f.data(), f.size(), flags_before, flags_after, out, cap);
}
int hd_host_ax25_format(const uint8_t* data, size_t n, char* out, size_t cap)
{
    if (!data || !out || !cap) return HD_ERR_INVALID;
    std::string s;
    if (const int rc = hd::ax25_format(data, n, s)) return rc;
    if (s.size() + 1 > cap) return HD_ERR_CAPACITY;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}

/* ---- baud-rate probe (kernels/baud_probe.hip; see host/baud_probe.hpp) ---- */
struct hd_host_baud_probe {
    hd_baud_probe_params prm;
    hd::BaudProbeTables t;
    hd::BaudProbeStream s;
};
hd_host_baud_probe* hd_host_baud_probe_new(double decimated_rate, const hd_baud_probe_params* params)
{
    hd_baud_probe_params prm;
    hd::baud_probe_params_default(&prm);
    if (params) prm = *params;
    if (!hd::baud_probe_params_ok(&prm, decimated_rate)) return nullptr;
    auto* h = new hd_host_baud_probe;
    h->prm = prm;
    h->t.make(decimated_rate, prm);
    return h;
}
void hd_host_baud_probe_free(hd_host_baud_probe* h) { delete h; }
void hd_host_baud_probe_reset(hd_host_baud_probe* h) { if (h) h->s.reset(); }
void hd_host_baud_probe_push(hd_host_baud_probe* h, const float* d, size_t n) { if (h && d && n) h->s.push(h->t, d, n); }
int hd_host_baud_probe_state(const hd_host_baud_probe* h, hd_baud_probe_stream_state* hdr, hd_baud_probe_candidate* candidates, size_t cap)
{
    if (!h) return HD_ERR_INVALID;
    if (cap < hd::kProbeCand) return (int)hd::kProbeCand;
    if (hdr) *hdr = h->s.h;
    if (candidates) std::memcpy(candidates, h->s.c.data(), hd::kProbeCand * sizeof(hd_baud_probe_candidate));
    return (int)hd::kProbeCand;
}
int hd_host_baud_probe_estimate(const hd_host_baud_probe* h, hd_baud_estimate* out)
{
    if (!h || !out) return HD_ERR_INVALID;
    hd::baud_probe_estimate(h->t, h->prm, h->s.h, h->s.c.data(), out);
    return HD_OK;
}

/* ---- framing trial (see host/format_trial.hpp) ---- */
struct hd_host_format_trial { hd::FormatTrial f; };
hd_host_format_trial* hd_host_format_trial_new(void) { return new hd_host_format_trial; }
void hd_host_format_trial_free(hd_host_format_trial* h) { delete h; }
void hd_host_format_trial_push_bits(hd_host_format_trial* h, const uint8_t* bits, size_t n) { if (h && (bits || !n)) h->f.push_bits(bits, n); }
void hd_host_format_trial_get(const hd_host_format_trial* h, hd_format_trial_result* out) { if (h && out) h->f.get(out); }

}  // extern "C"
