/*
 * habdec_amd_host.h -- C ABI of the HOST-side pieces of the path (no GPU needed to call these).
 *
 * They are the exact routines the engine uses around its kernels: the decimation plan and coefficient tables,
 * the low-pass design, RTTY framing, sentence extraction + CRC, the AFC state machine, and the float-only
 * atan2f restatement the discriminator kernel runs.  Exported so integrators and the CPU test-suite can drive
 * them directly; each names the reference routine it stands in for.
 */
#ifndef HABDEC_AMD_HOST_H
#define HABDEC_AMD_HOST_H
#include <stddef.h>
#include <stdint.h>

#include "habdec_amd.h"   /* hd_survey_params, hd_survey_candidate */
#ifdef __cplusplus
extern "C" {
#endif

/* Decoder::setupDecimationStagesFactor's stage choice (Decoder.h:286-320): returns the stage count (0..2) or -1;
 * ratio[i], ntaps[i] describe stage i. */
int hd_host_decim_plan(unsigned total_factor, int ratio[2], unsigned ntaps[2]);
/* coefficients of stage `stage` of that plan (filtercoef.h tables); returns the count copied */
size_t hd_host_decim_taps(unsigned total_factor, int stage, float* taps, size_t cap);

/* FirFilter::LP_BlackmanHarris (FirFilter.h:173-209): design for `batch` input samples; `prev_ntaps` is the tap
 * count currently in use (a design of equal length is skipped -> returns 0).  float_trig: DESIGN.md lookup context. */
size_t hd_host_lowpass_design(float cutoff_rel, float transition, size_t batch, size_t prev_ntaps, int float_trig,
                              float* taps, size_t cap);

/* The LDS a low-pass launch needs (kernels/fir_demod.hip: a tile's inputs for ALL taps of the longest filter of the call live in LDS), and its inverse.
 * hd_host_fir_demod_lds_bytes: dynamic LDS bytes of a launch whose longest filter has `taps` taps; *static_bytes (optional) receives the kernel's static LDS,
 * which the launch needs on top.  hd_host_fir_demod_max_taps: the largest odd tap count whose launch, dynamic and static together, fits `lds_bytes`
 * (0: none) -- 6611 for 64 KB, 18899 for the 160 KB of a gfx950 CU.  The engine derives hd_engine_lowpass_taps_max from it and the device's LDS per workgroup. */
size_t hd_host_fir_demod_lds_bytes(uint32_t taps, size_t* static_bytes);
uint32_t hd_host_fir_demod_max_taps(size_t lds_bytes);

/* RTTY<bool> (RTTY.h:59-137) */
typedef struct hd_host_rtty hd_host_rtty;
hd_host_rtty* hd_host_rtty_new(size_t nbits, float nstops);
void hd_host_rtty_free(hd_host_rtty*);
size_t hd_host_rtty_push_run(hd_host_rtty*, const uint8_t* bits, size_t n, char* out, size_t cap);
size_t hd_host_rtty_pending(const hd_host_rtty*);   /* unframed bits the framer still holds (bounded: 2^18 + what can still frame) */

/* CRC (CRC.cpp:21-47) and extractSentence (sentence_extract.cpp:58-98) */
void hd_host_crc16(const char* s, size_t n, char out4[5]);
int hd_host_extract_sentence(const char* stream, size_t n, char* callsign, char* data, char* crc, char* rest, size_t cap);

/* Decoder text stage (Decoder.h:568-637) on raw framed bytes */
typedef struct hd_host_text hd_host_text;
hd_host_text* hd_host_text_new(size_t nbits, float nstops);
void hd_host_text_free(hd_host_text*);
void hd_host_text_push_bits(hd_host_text*, const uint8_t* bits, size_t n);
size_t hd_host_text_get(hd_host_text*, int which /*0 rtty stream,1 last sentence,2 ok log,3 match log,4 chars log*/, char* buf, size_t cap);

/* AFC::process after the spectrum reductions (AFC.h:108-184) + resetFrequencyCorrection (AFC.h:187-194) */
typedef struct hd_host_afc hd_host_afc;
hd_host_afc* hd_host_afc_new(void);
void hd_host_afc_free(hd_host_afc*);
void hd_host_afc_step(hd_host_afc*, int have_spectrum, int valid, int peak1, int peak2, float power1, float power2,
                      double mean, double sigma, size_t bins, double rate);
void hd_host_afc_reset(hd_host_afc*, double correction, size_t bins, double rate);
void hd_host_afc_get(hd_host_afc*, double* correction, double* shift_hz, double* noise_floor, double* noise_sigma,
                     int* peak_l, int* peak_r);

/* the discriminator's arithmetic, compiled for the host: bit-identical to glibc atan2f (FSK2_Demod.h:38) */
void hd_host_atan2f(const float* y, const float* x, float* out, size_t n);
void hd_host_discriminate(const float* iq, size_t n, float prev_re, float prev_im, float* out);

/* ---- GUI payloads: the websocket server's binary "PWR_" / "DEM_" bodies, per stream ----
 * hd_host_spectrum_payload = SpectrumToStream (habdec_ws_protocol.cpp:355-405): zoom to the centre bins (zoom clamped to
 * [0.01, 0.99]), thin to `resolution` bins (ShrinkVector, :338-351), quantise to type_size 1/2/4 bytes per bin against the
 * slice's min/max (CompressedVector.cpp:75-118), behind the 52-byte SpectrumInfoHeader (NetTransport.h:29-47).  `bins` is
 * hd_stream_power(), the scalars are hd_stream_afc() (peak_left/right signed like AFC::getPeaks) and the decimated rate.
 * hd_host_demod_payload = DemodToStream + the 20-byte DemodHeader (:408-429, NetTransport.h:50-57) for hd_stream_demodulated().
 * Both return the payload size in bytes (written to `out` when cap suffices) and the number of values sent. */
size_t hd_host_spectrum_payload(const float* bins, size_t n, double noise_floor, double noise_variance, double sampling_rate, double shift,
                                int peak_left, int peak_right, float zoom, int resolution, int type_size, uint8_t* out, size_t cap,
                                size_t* bins_sent);
size_t hd_host_demod_payload(const float* trace, size_t n, int resolution, int type_size, uint8_t* out, size_t cap, size_t* values_sent);

/* ---- post-decode telemetry ----
 * Return convention of the parsers: 1 = parsed, 0 = the reference returns "nothing" (std::nullopt / no GPS fix / fewer than
 * six fields), -1 = an input on which the reference lets std::stoi / std::stof / std::string::at throw. */
typedef struct hd_host_telemetry {
    char callsign[64];            /* leading '$' run removed (sentence_parse.cpp:156-163) */
    int32_t frame, hour, minute;
    float second, lat, lon, alt;  /* decimal degrees; NMEA ddmm.mmmm inputs converted (sentence_parse.cpp:106-143) */
} hd_host_telemetry;
int hd_host_parse_time(const char* text, int* hour, int* minute, float* second);             /* parse_sentence_time, :47-68 */
int hd_host_parse_gps_pos(const char* text, float* out);                                      /* parse_gps_pos, :106-143 */
int hd_host_parse_sentence(const char* sentence_without_crc, hd_host_telemetry* out);         /* parse_sentence, :146-196, without the clock */
/* timestamp_from_HMS (:73-100) with the clock passed in (seconds since the epoch, UTC): "YYYY-MM-DDTHH:MM:SSZ" */
size_t hd_host_timestamp_from_hms(int64_t now_unix, int hour, int minute, float second, char* buf, size_t cap);
/* CalcGpsDistance (GpsDistance.cpp:21-84): out = {line distance m, great-circle distance m, angle rad, elevation deg, bearing deg} */
void hd_host_gps_distance(double lat1, double lon1, double alt1, double lat2, double lon2, double alt2, double out[5]);

/* ---- sondehub upload batch (last hop): the JSON body of SondeHubUploader::upload (sondehub_uploader.cpp:31-69) ----
 * Any number of threads push (one record per CRC-valid sentence: what SentenceCallback does, websocketServer/main.cpp:286-306 --
 * habdec::parse_sentence, time_received = utc_now_iso()); one thread takes the batch: a JSON array with the reference's eleven fields per
 * record, serialised byte for byte like its nlohmann::json (keys sorted, compact, Grisu2 shortest floats, alt as int).  The HTTP PUT
 * itself is the application's.  Clocks are passed in (nanoseconds since the epoch, UTC), so results are reproducible. */
typedef struct hd_host_sondehub hd_host_sondehub;
hd_host_sondehub* hd_host_sondehub_new(const char* uploader_callsign, const char* software_version /* first 7 characters are used */);
void hd_host_sondehub_free(hd_host_sondehub*);
/* 1 = queued; 0 = dropped like the reference does (fewer than six fields, no GPS fix, bad time); -1 = the reference would throw (stoi / stof) */
int hd_host_sondehub_push_sentence(hd_host_sondehub*, uint32_t stream, const char* callsign, const char* data, int64_t now_unix_ns);
int hd_host_sondehub_push(hd_host_sondehub*, const char* payload_callsign, const char* time_received, const char* datetime, int frame,
                          float lat, float lon, float alt);                                   /* SondeHubUploader::push of a ready MinTelemetry */
size_t hd_host_sondehub_size(const hd_host_sondehub*);
/* Body size in bytes (0 = queue empty); written NUL-terminated to out when cap > size, and only then is the batch consumed. */
size_t hd_host_sondehub_take(hd_host_sondehub*, int64_t now_unix_ns, char* out, size_t cap, size_t* n_records);
size_t hd_host_utc_iso(int64_t unix_ns, char* buf, size_t cap);                              /* utc_now_iso() (common/utc_now_iso.cpp:7-22) at a given instant */
size_t hd_host_json_number(double v, char* buf, size_t cap);                                 /* how the body prints a float field */

/* ---- batched cf32 file ingest: S IQ files -> one push slab per round ----
 * Each file is an IQSource_File<float> (IQSource_File.h:124-172): raw interleaved float32 I,Q, no header; a read returns
 * what is left, the end of file is noticed by the read that runs into it, and the NEXT read rewinds when `loop` (else
 * returns 0).  `chunk` = samples requested per stream and round (the reference asks for 65536, main.cpp:235);
 * `granule` = the decoder's total decimation factor: every stream delivers a whole multiple of it per round and the
 * remainder is carried in front of its next round (what Decoder::process does with its queue, Decoder.h:429-435).
 * `realtime_rate` > 0 throttles each round like IQSource_File.h:165-169; 0 = as fast as the files can be read. */
typedef struct hd_host_iqfiles hd_host_iqfiles;
hd_host_iqfiles* hd_host_iqfiles_open(const char* const* paths, uint32_t n_files, int loop, uint32_t chunk, uint32_t granule,
                                      double realtime_rate);
void hd_host_iqfiles_close(hd_host_iqfiles*);
uint32_t hd_host_iqfiles_streams(const hd_host_iqfiles*);
uint64_t hd_host_iqfiles_count(const hd_host_iqfiles*, uint32_t stream);     /* IQSource_File::count(): samples in the file */
uint64_t hd_host_iqfiles_rewinds(const hd_host_iqfiles*, uint32_t stream);
/* One round: slab[s*stride .. ] (stride in complex samples, >= chunk) receives stream s's samples, n_per_stream[s] how many
 * (a multiple of granule).  Returns the number of streams that read anything (0: all files exhausted and not looping). */
uint32_t hd_host_iqfiles_next(hd_host_iqfiles*, float* slab, size_t stride, uint32_t* n_per_stream);
/* Packed files (HD_IQ_*, include/habdec_amd.h): the same reader over raw cs16 / cs8 / cu8 files -- count = file size / bytes per sample; reads, the
 * granule carry and rewinds are counted in samples and hold packed bytes.  hd_host_iqfiles_open is hd_host_iqfiles_open_fmt(..., HD_IQ_CF32); NULL for an
 * unknown fmt.  hd_host_iqfiles_next on a packed batch delivers the converted floats (hd_host_iq_convert); hd_host_iqfiles_next_raw fills the slab with the
 * file's own bytes (stride still in complex samples: stream s starts at byte s * stride * hd_host_iq_bytes(fmt)) -- what hd_ingest_run hands on packed.
 * Either call advances the batch by one round. */
hd_host_iqfiles* hd_host_iqfiles_open_fmt(const char* const* paths, uint32_t n_files, int loop, uint32_t chunk, uint32_t granule,
                                          double realtime_rate, int fmt);
uint32_t hd_host_iqfiles_next_raw(hd_host_iqfiles*, void* slab, size_t stride, uint32_t* n_per_stream);
/* The packed formats on the host, for checks without a GPU: bytes per complex sample (0 = unknown fmt), and the conversion the GPU performs --
 * `n` complex samples at `src` (any alignment; exactly n * bytes are read) to 2 n floats at `out`.  An unknown fmt writes nothing. */
size_t hd_host_iq_bytes(int fmt);
void hd_host_iq_convert(int fmt, const void* src, size_t n, float* out);

/* ---- per-stream digital tuning (hd_stream_set_tune, include/habdec_amd.h): the arithmetic the kernels run, for checks without a GPU ----
 * hd_host_tune_step: step = (uint32_t)(int64_t)nearbyint(-(offset_hz / decimated_rate) * 2^32), rounded half to even; HD_ERR_INVALID (-1) unless
 * |offset_hz| < decimated_rate / 2.  hd_host_tune_tables: coarse[2a], coarse[2a+1] = (cos, sin)(2 pi a / 256), fine[2b], fine[2b+1] =
 * (cos, sin)(2 pi b / 65536), a, b < 256, computed in double and rounded to float once.  hd_host_tune_rotate: out[i] = iq[i] * C[theta >> 24] *
 * F[(theta >> 16) & 255] with theta = phase + i * step (mod 2^32), interleaved (I, Q) floats, every product and sum rounded separately (no FMA);
 * out may equal iq. */
int  hd_host_tune_step(double offset_hz, double decimated_rate, uint32_t* step);
void hd_host_tune_tables(float coarse[512], float fine[512]);
void hd_host_tune_rotate(const float* iq, size_t n, uint32_t phase, uint32_t step, float* out);

/* ---- wideband survey (hd_survey_*, include/habdec_amd.h): the window the kernel multiplies by, and the detector ----
 * hd_host_survey_window: w[n] = 0.5 - 0.5 cos(2 pi n / 4096) (periodic Hann), computed in double and rounded to float once.
 * hd_host_survey_detect: a pure function of a 4096-bin averaged power spectrum (power[i] at f_i = (i - 2048) sampling_rate / 4096).  In order:
 *  1. segments < 16 is HD_ERR_UNSUPPORTED (a threshold means nothing over a handful of periodograms); a NaN or negative power, threshold_db < 0 or a
 *     negative Hz parameter is HD_ERR_INVALID (so are null arguments, and a guard that leaves no bin); a floor of 0 is HD_ERR_UNSUPPORTED.
 *  2. Eligible bins: those with |f| >= dc_guard_hz (all when it is 0).  floor = their median (the mean of the two middle values of the sorted list).
 *  3. An eligible bin is marked when P >= floor * max(10^(threshold_db / 10), 1 + 8 / sqrt(segments)); the second term is where noise alone ends.
 *  4. Marked bins form one cluster while at most g = ceil(merge_hz / (sampling_rate / 4096)) unmarked bins lie between neighbours (index difference
 *     <= g + 1); no wrap-around between bin 4095 and bin 0.
 *  5. Over a cluster's marked bins: offset_hz = sum f_i (P_i - floor) / sum (P_i - floor), snr_db = 10 log10(sum (P_i - floor) / floor),
 *     width_hz = (bin_hi - bin_lo + 1) sampling_rate / 4096; clusters wider than max_width_hz are dropped when it is > 0.
 *  6. Sorted by snr_db descending, ties by lower offset_hz; *found = clusters, the first min(found, cap) are written. */
void hd_host_survey_window(float w[4096]);
int  hd_host_survey_detect(const double* power, uint64_t segments, double sampling_rate, const hd_survey_params* p, hd_survey_candidate* out,
                           uint32_t cap, uint32_t* found);

/* ---- waterfall (hd_waterfall_*, include/habdec_amd.h has the contract): the row detector and the tracker in plain C++ ----
 * hd_host_waterfall_detect_row: the detector's steps 1-6 on one row of 4096 float sums of `segments` (1..64) segments; of p only threshold_db and
 *   dc_guard_hz are looked at.  Writes hdr->segments, flags, floor, level and n_marked (first_sample and _pad = 0) and the 128 mark words -- bit for bit
 *   what the GPU's detector leaves for the same row.  Null arguments, segments outside 1..64, sampling_rate <= 0, a negative or NaN parameter or a guard
 *   that leaves no bin: HD_ERR_INVALID.
 * hd_host_waterfall_tracks: the tracker over headers[n_rows] and marks[n_rows][128] (hd_waterfall_tracks calls it with the rows it keeps).  Null
 *   arguments (out may be null when cap is 0; headers and marks when n_rows is 0), sampling_rate <= 0, a negative or NaN merge_hz or max_width_hz:
 *   HD_ERR_INVALID. */
void hd_host_waterfall_params_default(hd_waterfall_params* p);
int  hd_host_waterfall_detect_row(const float* row, uint32_t segments, double sampling_rate, const hd_waterfall_params* p, hd_waterfall_row* hdr,
                                  uint32_t* marks);
int  hd_host_waterfall_tracks(const hd_waterfall_row* headers, const uint32_t* marks, uint64_t n_rows, double sampling_rate,
                              const hd_waterfall_track_params* p, hd_waterfall_track* out, uint32_t cap, uint32_t* found);

/* ---- baud-rate probe (hd_baud_probe_*, include/habdec_amd.h has the definition): one stream of it in plain C++, sample by sample ----
 * The same structs and the same integers as the kernel: hd_host_baud_probe_state of the same pushes equals hd_baud_probe_state bit for bit, and
 * hd_baud_probe_estimate is a copy of the device state followed by the estimate of this file.  `decimated_rate` = fsd; params null: the defaults;
 * NULL for parameters hd_baud_probe_create refuses.  hd_host_baud_probe_state returns HD_PROBE_CANDIDATES and writes nothing at all when cap is smaller. */
typedef struct hd_host_baud_probe hd_host_baud_probe;
hd_host_baud_probe* hd_host_baud_probe_new(double decimated_rate, const hd_baud_probe_params* params);
void hd_host_baud_probe_free(hd_host_baud_probe*);
void hd_host_baud_probe_reset(hd_host_baud_probe*);
void hd_host_baud_probe_push(hd_host_baud_probe*, const float* d, size_t n);
int  hd_host_baud_probe_state(const hd_host_baud_probe*, hd_baud_probe_stream_state* hdr, hd_baud_probe_candidate* candidates, size_t cap);
int  hd_host_baud_probe_estimate(const hd_host_baud_probe*, hd_baud_estimate* out);

/* ---- framing trial (hd_stream_set_format_trial, include/habdec_amd.h): four hd_host_text chains (7N1, 7N2, 8N1, 8N2) over the same bits ---- */
typedef struct hd_host_format_trial hd_host_format_trial;
hd_host_format_trial* hd_host_format_trial_new(void);
void hd_host_format_trial_free(hd_host_format_trial*);
void hd_host_format_trial_push_bits(hd_host_format_trial*, const uint8_t* bits, size_t n);
void hd_host_format_trial_get(const hd_host_format_trial*, hd_format_trial_result* out);

/* ---- clocked decoder (hd_clocked_*, include/habdec_amd.h has the definition): one stream of it in plain C++, position by position ----
 * The same structs and the same integers as the kernel: the records of the same pushes equal hd_clocked_records byte for byte, and the text stage and
 * the repair behind them are the code the engine's object runs.  hd_host_clocked_new: NULL for parameters hd_clocked_create refuses; the stream is off
 * until hd_host_clocked_set_modem (HD_ERR_UNSUPPORTED where hd_clocked_set_modem is) gives it a modem.  The other calls as their hd_clocked_* namesakes.
 * hd_host_chase_repair: the repair alone on a span of n characters with data[n][8] their data_k -- 1 and out[n], *flips when a trial counts, 0 when
 * none does (out untouched), HD_ERR_INVALID for null arguments, nbits other than 7 or 8, repair_bits > 16 or repair_flips > 4. */
typedef struct hd_host_clocked hd_host_clocked;
hd_host_clocked* hd_host_clocked_new(double decimated_rate, const hd_clocked_params* params);
void hd_host_clocked_free(hd_host_clocked*);
void hd_host_clocked_reset(hd_host_clocked*);
int  hd_host_clocked_set_modem(hd_host_clocked*, double baud, uint32_t nbits, uint32_t nstops, int invert);
void hd_host_clocked_push(hd_host_clocked*, const float* d, size_t n);
int  hd_host_clocked_records(hd_host_clocked*, hd_clocked_record* out, size_t cap);
int  hd_host_clocked_take_sentences(hd_host_clocked*, hd_clocked_sentence* out, size_t cap);
int  hd_host_clocked_stats(const hd_host_clocked*, hd_clocked_counters* out);
int  hd_host_chase_repair(const char* span, size_t n, const int32_t* data, uint32_t nbits, uint32_t repair_bits, uint32_t repair_flips, char* out,
                          uint32_t* flips);

/* ---- tone-filter demodulator (hd_tones_*, include/habdec_amd.h has the definition): one stream of it in plain C++, sample by sample ----
 * The same integers as the kernel: the rows of the same pushes equal the device rows byte for byte.  hd_host_tones_new: NULL unless decimated_rate > 0
 * (params null: the defaults); the stream has no modem until hd_host_tones_set_modem gives it one, with the errors of hd_tones_set_modem.
 * hd_host_tones_push takes n cf32 samples at iq (2 n floats), writes n floats to out and returns n; without a modem it writes nothing and returns 0.
 * hd_host_tones_stats as hd_tones_stats. */
typedef struct hd_host_tones hd_host_tones;
hd_host_tones* hd_host_tones_new(double decimated_rate, const hd_tones_params* params);
void   hd_host_tones_free(hd_host_tones*);
void   hd_host_tones_reset(hd_host_tones*);
int    hd_host_tones_set_modem(hd_host_tones*, double baud, double f_hi_hz, double f_lo_hz);
size_t hd_host_tones_push(hd_host_tones*, const float* iq, size_t n, float* out);
int    hd_host_tones_stats(const hd_host_tones*, hd_tones_info* out);

/* ---- tone search (hd_tone_search_*, include/habdec_amd.h has the spectrum's definition): the detector, and one stream of the spectrum ----
 * hd_host_tone_search_detect: a pure function of a 4096-bin averaged power spectrum P (P[k] at (k - 2048) fsd / 4096) of `segments` segments.  All
 * arithmetic in double, every sum sequential in ascending index.  In order:
 *  1. Null arguments, baud <= 0, fsd <= 0, shift_lo_hz <= 0, shift_hi_hz < shift_lo_hz, min_quality < 0, a NaN or an Inf among them: HD_ERR_INVALID.
 *     Fewer than 8 segments: HD_ERR_UNSUPPORTED.
 *  2. bin = fsd / 4096.  w = max(1, nearbyint(0.5 baud / bin)) | 1 (odd), h = w / 2: the bins one tone's window holds.  The spacings searched are
 *     d = ceil(shift_lo_hz / bin) .. min(floor(shift_hi_hz / bin), 4096 - w); no such d, or w >= 4096: HD_ERR_INVALID.
 *  3. A non-finite P: HD_OK with valid = 0; w and segments are set, every other field is 0.
 *  4. floor = the median of the 4096 values (the mean of the two middle ones).
 *  5. B[k] = sum over k - h <= m <= k + h of (P[m] - floor), for h <= k < 4096 - h.
 *  6. Coarse search: d ascending, then lo from h to 4096 - h - d - 1 ascending; score = min(B[lo], B[lo + d]); the first strictly greatest score
 *     wins (bin_lo, shift_bins).  The minimum is deliberate: both tones must be there, a lone carrier scores like noise.
 *  7. Refinement of each of the two bins c = bin_lo, bin_lo + shift_bins, three rounds: r = max(1, nearbyint(0.3 baud / bin)); weights
 *     max(P[m] - floor, 0) over c - r <= m <= c + r clamped to the array; cf = the weighted centroid (c itself when the weights sum to 0);
 *     c = nearbyint(cf), ties to even.  The tone is (cf - 2048) bin of the last round: f_lo_hz from bin_lo, f_hi_hz from the other.
 *  8. quality = score / (w floor), 0 when floor <= 0.  valid = 1 when floor > 0 and quality >= max(min_quality, 10 / sqrt(w segments)); noise alone
 *     stayed below 6.1 / sqrt(w segments) where it was measured (NOTES.md).
 * hd_host_tone_search_create / _push / _power / _reset / _destroy: one stream of the spectrum in plain C++ -- the same segmentation over the absolute
 * sample index and the same float window products, then a double-precision transform and |X|^2 in double; hd_host_tone_search_push takes n cf32 samples
 * (2 n floats); hd_host_tone_search_power as hd_tone_search_power.  The GPU's accumulators agree with it to the float transform's error, not byte for byte. */
typedef struct hd_host_tone_search hd_host_tone_search;
int    hd_host_tone_search_detect(const double* p, uint64_t segments, double fsd, const hd_tone_search_detect_params* params, hd_tone_search_result* out);
hd_host_tone_search* hd_host_tone_search_create(void);
void   hd_host_tone_search_destroy(hd_host_tone_search*);
void   hd_host_tone_search_reset(hd_host_tone_search*);
void   hd_host_tone_search_push(hd_host_tone_search*, const float* iq, size_t n);
int    hd_host_tone_search_power(const hd_host_tone_search*, double* p, size_t cap, uint64_t* segments);

/* ---- diversity combiner (hd_combine_*, include/habdec_amd.h has the definition): one group of it in plain C++, sample by sample and lag by lag ----
 * The same integers as the kernels: rows, scores and results of the same pushes equal the device's byte for byte.  hd_host_combine_create: a group of
 * `count` members named by `streams` (the reference first; the names only label the results), NULL unless 1 <= count <= 8 and the names are distinct;
 * every delay 0, every weight 256.  Members are addressed by their position m in the group.  hd_host_combine_push: member m brings n_per_member[m]
 * (null: n) floats at rows + m * stride; unequal lengths are HD_ERR_INVALID and nothing is counted; n floats are written to out.  hd_host_combine_lags /
 * _align as hd_combine_lags / hd_combine_align; hd_host_combine_scores copies member m's (m >= 1) 2 L + 1 scores of the last search and returns their
 * number (0 before a search; nothing is written where cap is below it).  hd_host_combine_stats as hd_combine_stats. */
typedef struct hd_host_combine hd_host_combine;
hd_host_combine* hd_host_combine_create(const uint32_t* streams, uint32_t count);
void   hd_host_combine_destroy(hd_host_combine*);
void   hd_host_combine_reset(hd_host_combine*);
int    hd_host_combine_set_delay(hd_host_combine*, uint32_t m, uint32_t delay);
int    hd_host_combine_set_weight(hd_host_combine*, uint32_t m, uint32_t weight);
int    hd_host_combine_push(hd_host_combine*, const float* rows, size_t stride, const uint32_t* n_per_member, uint32_t n, float* out);
int    hd_host_combine_lags(hd_host_combine*, const hd_combine_lag_params* p, hd_combine_lag* out, size_t cap);
int    hd_host_combine_align(hd_host_combine*, const hd_combine_lag_params* p, hd_combine_lag* out, size_t cap);
int    hd_host_combine_scores(const hd_host_combine*, uint32_t m, int32_t* out, size_t cap);
int    hd_host_combine_stats(const hd_host_combine*, uint32_t m, hd_combine_info* out);

/* ---- SSDV packets (hd_ssdv_*, include/habdec_amd.h has the definition): one stream of it in plain C++, candidate by candidate ----
 * The doors, the gap rule, the delivery and the counters are the code the engine's object runs; the decoder restates the kernel by another route (log
 * tables, Berlekamp-Massey with an inverse) and the same pushes give the same packets and counters byte for byte.  hd_host_ssdv_create: NULL for
 * parameters hd_ssdv_create refuses.  Every push door scans.  hd_host_ssdv_encode: the 32 parity bytes (bytes 224 .. 255) of 223 data bytes.
 * hd_host_ssdv_make_packet: sync byte, type, the header fields, 205 payload bytes, CRC-32 and parity; a packet of type 0x67 (no-FEC) carries zeros where
 * the parity would be.  The callsign: its first 6 characters count, letters in either case and digits; any other character is stored as digit 0 and
 * reads back as '-'. */
typedef struct hd_host_ssdv hd_host_ssdv;
hd_host_ssdv* hd_host_ssdv_create(const hd_ssdv_params* params);
void   hd_host_ssdv_destroy(hd_host_ssdv*);
void   hd_host_ssdv_reset(hd_host_ssdv*);
int    hd_host_ssdv_push_bytes(hd_host_ssdv*, const uint8_t* bytes, const uint32_t* conf, size_t n);
int    hd_host_ssdv_push_records(hd_host_ssdv*, const hd_clocked_record* records, size_t n, uint32_t char_len);
int    hd_host_ssdv_take_packets(hd_host_ssdv*, hd_ssdv_packet* out, size_t cap);
int    hd_host_ssdv_stats(const hd_host_ssdv*, hd_ssdv_counters* out);
void   hd_host_ssdv_encode(const uint8_t* data223, uint8_t* parity32);
void   hd_host_ssdv_make_packet(uint8_t type, const char* callsign, uint8_t image_id, uint16_t packet_id, uint16_t width, uint16_t height, uint8_t flags,
                                uint8_t mcu_offset, uint16_t mcu_index, const uint8_t* payload205, uint8_t* out256);

/* ---- Horus Binary 4FSK (hd_fsk4_*, include/habdec_amd.h has the definition): one stream of it in plain C++, sample by sample, candidate by candidate ----
 * The same integers as the kernels: slot records, candidate records, frames and counters of the same samples equal the device's byte for byte, however
 * the samples are cut into pushes.  Selection, delivery and counters are the code the engine's object runs.  hd_host_fsk4_new: NULL unless
 * decimated_rate > 0 and the parameters are ones hd_fsk4_create takes (max_push 0: 4096).  hd_host_fsk4_set_modem: the errors of hd_fsk4_set_modem.
 * hd_host_fsk4_push: n cf32 samples (2 n floats), then a scan; 0 without a modem.  hd_host_fsk4_slots: the records of the slots first .. first + n - 1
 * (4 n words) while the ring still holds them; returns how many it wrote.  hd_host_fsk4_candidates: takes the log of the candidates behind the
 * unique-word gate, oldest first (the log keeps the newest 65536); out null: how many wait.  hd_host_fsk4_encode: payload_bytes bytes at payload (the
 * caller's CRC included) -> the frame's 2 + B bytes at out, unique word first; returns their number, 0 for a frame the decoder cannot take.
 * hd_host_fsk4_crc16: the payload check over n bytes. */
typedef struct hd_host_fsk4 hd_host_fsk4;
hd_host_fsk4* hd_host_fsk4_new(double decimated_rate, const hd_fsk4_params* params);
void   hd_host_fsk4_free(hd_host_fsk4*);
void   hd_host_fsk4_reset(hd_host_fsk4*);
int    hd_host_fsk4_set_modem(hd_host_fsk4*, double baud, double f0_hz, double spacing_hz, const hd_fsk4_frame* frame);
size_t hd_host_fsk4_push(hd_host_fsk4*, const float* iq, size_t n);
int    hd_host_fsk4_take_frames(hd_host_fsk4*, hd_fsk4_rx* out, size_t cap);
int    hd_host_fsk4_stats(const hd_host_fsk4*, hd_fsk4_counters* out);
size_t hd_host_fsk4_slots(const hd_host_fsk4*, uint64_t first, uint32_t* out, size_t n);
int    hd_host_fsk4_candidates(hd_host_fsk4*, hd_fsk4_candidate* out, size_t cap);
size_t hd_host_fsk4_encode(const hd_fsk4_frame* frame, const uint8_t* payload, uint8_t* out);
uint32_t hd_host_fsk4_crc16(const uint8_t* bytes, size_t n);
/* hd_fsk4_retune and hd_fsk4_retune_stats of the one stream, with their rules and errors. */
int    hd_host_fsk4_retune(hd_host_fsk4*, double f0_hz, double spacing_hz, uint64_t at_sample);
int    hd_host_fsk4_retune_stats(const hd_host_fsk4*, hd_fsk4_retune_info* out);

/* ---- 4FSK tone tracker (hd_fsk4_track_*, include/habdec_amd.h has the definition) ----
 * hd_host_fsk4_comb_detect: steps 1 .. 9 on 4096 fftshifted sums; the same integers as k_fsk4_comb, byte for byte.  HD_ERR_UNSUPPORTED: a spacing below
 * 2 baud; HD_ERR_INVALID: nothing to search; the record is all zero then.  hd_host_fsk4_track_*: one stream of the tracker with the tone search's
 * double-precision spectrum (hd_host_tone_search_*), so its sums agree with the device's to the float transform's error, not to the bit; epochs, decay,
 * records and the retunes of an attached hd_host_fsk4 as the engine's object.  hd_host_fsk4_track_new: NULL unless decimated_rate > 0 and the parameters
 * are ones hd_fsk4_track_create takes.  hd_host_fsk4_track_records: all records since the last reset, oldest first; out null: how many.
 * hd_host_fsk4_track_acc: the 4096 sums. */
int    hd_host_fsk4_comb_detect(const double* acc, double decimated_rate, const hd_fsk4_comb_params* p, hd_fsk4_comb_record* out);
typedef struct hd_host_fsk4_track hd_host_fsk4_track;
hd_host_fsk4_track* hd_host_fsk4_track_new(double decimated_rate, const hd_fsk4_track_params* params);
void   hd_host_fsk4_track_free(hd_host_fsk4_track*);
void   hd_host_fsk4_track_reset(hd_host_fsk4_track*);
int    hd_host_fsk4_track_set_stream(hd_host_fsk4_track*, double baud, double spacing_lo_hz, double spacing_hi_hz, double f_lo_hz, double f_hi_hz);
void   hd_host_fsk4_track_attach(hd_host_fsk4_track*, hd_host_fsk4* modem);
void   hd_host_fsk4_track_push(hd_host_fsk4_track*, const float* iq, size_t n);
int    hd_host_fsk4_track_records(hd_host_fsk4_track*, hd_fsk4_track_est* out, size_t cap);
int    hd_host_fsk4_track_stats(const hd_host_fsk4_track*, hd_fsk4_track_info* out);
int    hd_host_fsk4_track_acc(const hd_host_fsk4_track*, double* out);

/* ---- AFSK / AX.25 (hd_afsk_*, include/habdec_amd.h has the definition): one stream of it in plain C++, sample by sample, candidate by candidate ----
 * The same integers as the kernels: slot records, candidate records, frames and counters of the same samples equal the device's byte for byte, however
 * the samples are cut into pushes.  Selection, delivery and counters are the code the engine's object runs.  hd_host_afsk_new: NULL unless
 * decimated_rate > 0 and the parameters are ones hd_afsk_create takes (max_push 0: 4096).  hd_host_afsk_set_modem: the errors of hd_afsk_set_modem.
 * hd_host_afsk_push: n floats, then a scan; 0 without a modem.  hd_host_afsk_slots: the records of the slots first .. first + n - 1 (n int32) while
 * the ring still holds them; returns how many it wrote.  hd_host_afsk_candidates: takes the log of the candidates, oldest first (the log keeps the newest
 * 16384); out null: how many wait.  hd_host_afsk_crc16: the FCS of n bytes.
 * AX.25 UI frames.  path is the TNC2 header, "SRC-SSID>DST,DIGI1,DIGI2*" (callsigns of 'A'-'Z', '0'-'9', SSID 0 .. 15, at most eight digipeaters, '*'
 * sets a digipeater's H bit).  hd_host_ax25_frame: addresses, control 0x03, PID 0xF0, info, FCS -> the frame's bytes; returns their number, 0 for a
 * path that is none or a capacity too small.  hd_host_ax25_levels: frame bytes (FCS included) -> flags_before flags, the stuffed bits, flags_after
 * flags as NRZI levels, one byte (0 / 1) a bit, the level in front of the first bit 0; returns their number and writes them where they fit cap (out
 * null: the count alone).  hd_host_ax25_encode: both in one.  hd_host_ax25_format: a UI frame without its FCS -> the TNC2 monitor line
 * "SRC-SSID>DST,DIGI*:info" with its terminating 0, the '*' behind the last digipeater whose H bit is set, bytes outside 32 .. 126 as <0xNN>; returns
 * the line's length, HD_ERR_INVALID for an address field that fails the address check, HD_ERR_UNSUPPORTED for a frame that is not UI, HD_ERR_CAPACITY. */
typedef struct hd_host_afsk hd_host_afsk;
hd_host_afsk* hd_host_afsk_new(double decimated_rate, const hd_afsk_params* params);
void   hd_host_afsk_free(hd_host_afsk*);
void   hd_host_afsk_reset(hd_host_afsk*);
int    hd_host_afsk_set_modem(hd_host_afsk*, double baud, double mark_hz, double space_hz);
size_t hd_host_afsk_push(hd_host_afsk*, const float* row, size_t n);
int    hd_host_afsk_take_frames(hd_host_afsk*, hd_afsk_rx* out, size_t cap);
int    hd_host_afsk_stats(const hd_host_afsk*, hd_afsk_counters* out);
size_t hd_host_afsk_slots(const hd_host_afsk*, uint64_t first, int32_t* out, size_t n);
int    hd_host_afsk_candidates(hd_host_afsk*, hd_afsk_candidate* out, size_t cap);
uint32_t hd_host_afsk_crc16(const uint8_t* bytes, size_t n);
size_t hd_host_ax25_frame(const char* path, const uint8_t* info, size_t n_info, uint8_t* out, size_t cap);
size_t hd_host_ax25_levels(const uint8_t* frame, size_t n, uint32_t flags_before, uint32_t flags_after, uint8_t* out, size_t cap);
size_t hd_host_ax25_encode(const char* path, const uint8_t* info, size_t n_info, uint32_t flags_before, uint32_t flags_after, uint8_t* out, size_t cap);
int    hd_host_ax25_format(const uint8_t* data, size_t n, char* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
