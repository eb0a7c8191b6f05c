/*
 * habdec_amd.h -- C ABI of the MI355X-native RTTY demodulation engine (libhabdec_amd.so).
 *
 * This is the drop-in boundary underneath a source-compatible `habdec::Decoder<T>`
 * (habdec_amd/include/habdec/Decoder.h).  The reference has no FFI for this path -- its boundary is the
 * public surface of the header-only class template `habdec::Decoder<TReal>` (reference
 * code/Decoder/Decoder.h:65-141) -- so every entry point below names the reference member(s) it stands in
 * for.  Plain C types only: no C++, no torch, no HIP types cross this line.
 *
 * Model: one *engine* per GPU owns S independent *streams* (S = 1 for the websocket server's single
 * decoder, thousands for batch decoding).  All streams of an engine share the input sampling rate and
 * the decimation plan; baud / framing / low-pass settings are per stream.  One `hd_process_*` call is one
 * `pushSamples()+operator()()` round (reference code/websocketServer/main.cpp:240-245) for every stream.
 *
 * Threading: an engine is driven by ONE thread at a time for hd_process_* (like the reference's
 * DECODER_THREAD); getters/setters may be called from other threads and are serialised by an internal
 * mutex (reference Decoder.h:209,229,240,423).  Callbacks fire synchronously inside hd_process_*, in
 * stream order, on the calling thread (reference Decoder.h:604-606,625-626).
 *
 * Errors: every function returning `int` returns HD_OK (0) or a negative HD_ERR_*; hd_last_error() gives
 * the message of the last failure on the calling thread.  The reference itself reports problems by printing
 * and carrying on (Decoder.h:272-276, FirFilter.h:121-137); conditions it tolerates are tolerated here too,
 * conditions that are undefined behaviour there (an input shorter than a stage's history, Decimator.h:140-143)
 * are rejected with HD_ERR_UNSUPPORTED.
 */
#ifndef HABDEC_AMD_H
#define HABDEC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HD_OK 0
#define HD_ERR_INVALID (-1)      /* bad argument */
#define HD_ERR_DEVICE (-2)       /* HIP / rocFFT failure, or no gfx950 device */
#define HD_ERR_UNSUPPORTED (-3)  /* input the reference has undefined behaviour on */
#define HD_ERR_CAPACITY (-4)     /* more samples than the engine was sized for */

#define HD_FFT_BINS 4096         /* reference Decoder.h:162 fft_bins_cnt_ */

typedef struct hd_engine hd_engine;

typedef struct hd_engine_config {
    int32_t  device;            /* HIP device ordinal */
    uint32_t n_streams;         /* S >= 1 */
    uint32_t max_chunk;         /* most IQ samples one stream hands to one hd_process_* call (65536 in main.cpp:235) */
    double   sampling_rate;     /* IQVector::samplingRate() latched by the first pushSamples (Decoder.h:215-216) */
    uint32_t decimation;        /* total factor 1,2,4,...,256 = setupDecimationStagesFactor(2^dec) (Decoder.h:268-332) */
    /* per-stream defaults; reference defaults in websocketServer/GLOBALS.h:87-100 and Decoder.h:172-173 */
    double   baud;              /* Decoder::baud()           */
    uint32_t rtty_bits;         /* Decoder::rtty_bits()  7|8 */
    float    rtty_stops;        /* Decoder::rtty_stops() 1|2 */
    float    lowpass_bw_hz;     /* Decoder::lowpass_bw()     */
    float    lowpass_trans;     /* Decoder::lowpass_trans()  */
    int32_t  dc_remove;         /* Decoder::dc_remove()      */
    /* How the reference's unqualified sin/cos/abs calls resolved in the translation unit that compiled it
     * (DESIGN.md "lookup context"): 1 = <math.h> context (float trig in the tap design, float |.| in the
     * flip-point weights; default), 0 = <cmath>-only context (double trig, integer abs). */
    int32_t  lookup_mode;
    int32_t  enable_spectrum;   /* 1 = run the 4096-bin spectrum + AFC like the reference, 0 = skip (stage benchmarks) */
    /* 0 = keep the reference's decode gate: above 160 kHz decimated rate only decimation/FFT/AFC run
     * (Decoder.h:522-527).  1 = stage-level mode: FIR/demod/symbols run at any rate (BASELINE config 3). */
    int32_t  ungated;
    int32_t  keep_filtered;     /* 1 = also store the FIR output so hd_stream_filtered() works (parity tests) */
    /* 0 = hd_process_* returns after THIS call's text has been delivered (what Decoder::operator() does).
     * 1 = pipelined batch mode: a call enqueues its GPU work and delivers the PREVIOUS call's text, so the host
     *     text stage and the next call's decimation overlap the current call's symbol kernels; hd_flush() drains.
     * 2 = the same with one more call in flight where the launches of consecutive calls are strictly ordered on one queue (equally
     *     sized pushes through the step kernel): text arrives two calls late, and a host thread that is held up for the length of a
     *     launch does not leave the GPU idle.  Elsewhere 2 behaves like 1. */
    int32_t  pipeline;
    /* Arithmetic of the FIR sums (decimator stages Decimator.h:128-138, low-pass FirFilter.h:155-161).
     * 0 = HD_ARITH_EXACT (default): separately rounded multiply and add in ascending tap order, one accumulator per output -- every decimated, filtered
     *     and demodulated float is bit-identical to the reference's CPU arithmetic.
     * 1 = HD_ARITH_FAST: fused multiply-add (half the vector instructions of every FIR in the chain).  Intermediate floats agree with the exact mode to
     *     <= 1e-5 of the signal's peak, norm-wise per call.  Measured, per route: the decimator stages <= 3e-7; a low-pass as direct sums <= 7.6e-7
     *     (4097 taps); a low-pass of 1024 taps and more through transforms (the default from there on; HD_NO_LP_FFT=1 keeps the direct sums)
     *     6.6e-6 at 4097 taps, 8.4e-6 at 18899.  The discriminator and the symbol extractor are the exact mode's code, and on every stream of
     *     the parity suite the decoded characters and sentences are identical to the reference's -- streams that go to EXACT zeros and come back
     *     included, on every route (tests/test_gpu_fast_silence.py): a window of zeros sums to +0 as the reference's does, and a stream whose
     *     low-pass block holds a run of 64 samples that are exactly zero is filtered by direct sums in that call, not through the transforms, so where the
     *     reference filters exact zeros this mode does too and its discriminator output has the reference's bits there.
     *     Not bit-identical floats elsewhere: choose it for throughput. */
    int32_t  arith;
} hd_engine_config;
#define HD_ARITH_EXACT 0
#define HD_ARITH_FAST 1

/* Fill `cfg` with the reference defaults (dec 64, 300 baud 8N2, low-pass 1500 Hz / 0.025, spectrum on). */
void hd_engine_config_default(hd_engine_config* cfg);

/* Decoder construction + setupDecimationStagesFactor (Decoder.h:268-332) for S streams on one GPU. */
int  hd_engine_create(const hd_engine_config* cfg, hd_engine** out);
void hd_engine_destroy(hd_engine* e);
const char* hd_last_error(void);
/* Smallest non-empty per-stream sample count hd_process_* accepts at a decimation factor (a multiple of the factor that covers every stage's
 * history: shorter inputs are undefined behaviour in the reference's Decimator.h:140-143); 0 = unsupported factor.  A caller that drains a queue
 * (Decoder::process, Decoder.h:426-436) leaves fewer samples queued until more arrive. */
uint32_t hd_min_chunk(uint32_t decimation);
uint32_t hd_engine_streams(const hd_engine* e);
/* getDecimationFactor / getDecimatedSamplingRate (Decoder.h:716-735) */
uint32_t hd_engine_decimation(const hd_engine* e);
double   hd_engine_decimated_rate(const hd_engine* e);
/* The longest low-pass design a call may run, in taps.  The design follows the reference (FirFilter.h:185-188): size_t(4 / transition) taps, clamped to the
 * batch length of the call and forced odd -- so a narrow hd_stream_set_lowpass_trans makes the tap count follow the pushes.  The low-pass kernel keeps a
 * tile's inputs for all taps in LDS, so the limit is the smaller of
 *  - the engine's tap capacity (from max_chunk / decimation), and
 *  - the largest odd count whose launch fits the LDS the device grants one workgroup (habdec_amd_host.h: hd_host_fir_demod_max_taps; 18899 taps in the
 *    160 KB of an MI355X CU), never more than 65535.
 * One limit for both arithmetic modes.  A call in which some stream's design is longer is refused with HD_ERR_CAPACITY while it is planned: nothing is
 * queued, every stream stays as it was and the engine stays usable (widen the transition, or push less, and call again).
 * A change of the tap count between two runs of a stream reproduces the reference's stale-buffer transient exactly for a decrease and for an increase of
 * up to min(8192, m) taps, m = the batch length of the previous run: the first run with more taps takes, behind the kept history, the first samples of
 * the previous run's input, of which the engine keeps 8192.  A larger increase that does not restart the filter from zeros (the reference restarts when
 * its buffer grows) reads zeros where the reference reads older contents of its buffer: the first T - 1 outputs of that run (T = the new count) and what
 * the discriminator makes of them differ from the reference's; from output T - 1 on the run is the reference's again. */
uint32_t hd_engine_lowpass_taps_max(const hd_engine* e);

/* ---- per-stream control plane: the reference setters of the same names (Decoder.h:238-257, 655-712) ---- */
int hd_stream_set_baud(hd_engine* e, uint32_t stream, double baud);
int hd_stream_set_rtty(hd_engine* e, uint32_t stream, uint32_t bits, float stops);
int hd_stream_set_lowpass_bw(hd_engine* e, uint32_t stream, float hz);
int hd_stream_set_lowpass_trans(hd_engine* e, uint32_t stream, float trans);
int hd_stream_set_dc_remove(hd_engine* e, uint32_t stream, int on);
/* resetFrequencyCorrection (Decoder.h:806-809 -> AFC.h:187-194) */
int hd_stream_reset_frequency_correction(hd_engine* e, uint32_t stream, double correction);

/* ---- per-stream digital tuning and closed-loop AFC (not in the reference: its server retunes the radio instead, websocketServer/main.cpp:247-263) ----
 * A recording has no radio to retune, so the engine tunes each stream itself.  Stream s has an offset f (Hz), a phase step D and a phase P, both uint32 in
 * units of 2^-32 cycle; fs_dec = hd_engine_decimated_rate(e).
 *  - Where: the chunk the last decimation stage produces, after the DC blocker and before everything that reads the chunk (low-pass queue, spectrum feed,
 *    hd_stream_decimated).  The rest of the chain sees what a receiver tuned f higher would have delivered, within the decimators' passband: offsets
 *    near the band edge of the decimators are attenuated before the rotation.  The decimators' own state (history carries) stays unrotated.
 *  - Step: D = (uint32_t)(int64_t)nearbyint(-(f / fs_dec) * 2^32), rounded half to even; |f| >= fs_dec / 2 is HD_ERR_INVALID.
 *  - Phase: sample i (0 <= i < n2) of a call's chunk is rotated by theta = P + i D (mod 2^32); after the call P += n2 D.  A new offset takes effect from
 *    the first call submitted after it was set, the phase carries on without a jump.
 *  - Phasor: C[theta >> 24] * F[(theta >> 16) & 255], C[a] = (cos, sin)(2 pi a / 256), F[b] = (cos, sin)(2 pi b / 65536), built in double and rounded
 *    to float once; every complex product (ur vr - ui vi, ur vi + ui vr) with each product and sum rounded separately, in both arithmetic modes.
 *    Phase resolution 2^-16 cycle (spurs near -96 dBc).  habdec_amd_host.h restates it (hd_host_tune_*).
 *  - f = 0 sets D = P = 0, and a stream with D = 0 is not touched at all: bit-identical to an untuned stream on the same launch path.
 * Paths (hd_timing.path): the stream tail (2) and the step kernel (3) rotate in their stage-2 store, the separate kernels (0) in a per-chunk post-pass.
 * The band limit above -- (-fs_dec/2, fs_dec/2), and less near the decimators' band edge -- is what hd_stream_set_front_tune below lifts. */
int hd_stream_set_tune(hd_engine* e, uint32_t stream, double offset_hz);
/* Per-stream tuning at the INPUT rate, applied to a stream's IQ before the first decimation stage: one wideband recording fanned out (stream_stride = 0)
 * to streams whose payloads lie hundreds of kHz apart.  Df, Pf: uint32, units of 2^-32 cycle; fs = hd_engine_config.sampling_rate.
 *  - Step: Df = hd_host_tune_step(offset_hz, fs); |offset_hz| >= fs / 2 is HD_ERR_INVALID.  An engine with decimation 1 returns HD_ERR_UNSUPPORTED
 *    (hd_stream_set_tune is the same thing there).
 *  - Phase: input sample i (0 <= i < n) of a call is rotated by theta = Pf + i Df (mod 2^32); after the call Pf += n Df (a stream that brings n = 0 does
 *    not advance).  A new offset applies from the first call submitted after it was set; the phase carries on without a jump; nothing is drained.
 *  - Phasor: the one of hd_stream_set_tune (the same tables and roundings, in both arithmetic modes; hd_host_tune_rotate restates it).
 *  - Offset 0 sets Df = Pf = 0, and a stream with Df = Pf = 0 is not touched: bit-identical to an untuned stream on the same launch path.
 *  - Defining property: a front-tuned stream fed x is, in every float and every decoded character, a stream without front tuning fed
 *    hd_host_tune_rotate(x, Pf, Df) call by call -- also across a change of offset, on a first call, and on pushes so short that the first stage's
 *    history carry holds outputs: the first stage's history holds ROTATED samples.  Everything downstream (DC blocker, hd_stream_set_tune, the
 *    automatic AFC -- which keeps adjusting the decimated-rate offset only --, spectrum) sees the rotated input's decimation.
 *  - Paths: a call in which some stream has Df or Pf != 0 runs its first stage as a launch of its own with the rotation in its staging loop, then the
 *    stream tails (hd_timing.path 2) or the separate kernels (0); it never takes the step kernel (3) and reports step_variant 0.  When the last
 *    front offset goes back to 0 the next call is routed as before. */
int hd_stream_set_front_tune(hd_engine* e, uint32_t stream, double offset_hz);
typedef struct hd_front_tune_info {
    double   offset_hz;   /* current offset */
    uint32_t step, phase; /* Df, and Pf of the next call to be submitted */
    uint64_t from_call;   /* index (hd_process_* calls from 0) of the first call that used the current offset */
} hd_front_tune_info;
int hd_stream_front_tune(hd_engine* e, uint32_t stream, hd_front_tune_info* out);
/* The server's AFC block (websocketServer/main.cpp:247-263) counted in sample time, run per stream at each delivery right after the call's AFC step:
 * elapsed += the call's input samples; if on, elapsed >= hold_s * sampling_rate and |frequency correction| > min_hz, then f += correction (skipped when
 * |f + correction| >= fs_dec / 2), D is recomputed, the AFC is reset by the correction (hd_stream_reset_frequency_correction), elapsed = 0 and one retune
 * is counted.  The new offset applies to the first call submitted after that delivery: the next call at pipeline = 0, later in the pipelined modes by
 * the calls in flight (hd_tune_info.from_call says which).  Reference values: hold_s = 6 (the server's count() > 5 on whole seconds), min_hz = 100.
 * A retune does not drain the pipeline.  Setting the loop resets elapsed; turning it off keeps the current offset. */
int hd_stream_set_auto_afc(hd_engine* e, uint32_t stream, int on, double hold_s, double min_hz);
typedef struct hd_tune_info {
    double   offset_hz;   /* current offset: manual settings plus automatic retunes */
    uint32_t step, phase; /* D, and P of the next call to be submitted */
    uint64_t retunes;     /* automatic retunes so far */
    uint64_t from_call;   /* index (hd_process_* calls from 0) of the first call that used the current offset */
    int32_t  auto_afc;
} hd_tune_info;
int hd_stream_tune(hd_engine* e, uint32_t stream, hd_tune_info* out);

/* ---- callbacks: Decoder::sentence_callback_ / character_callback_ (Decoder.h:135-138) ---- */
typedef void (*hd_sentence_cb)(void* user, uint32_t stream, const char* callsign, const char* data, const char* crc);
typedef void (*hd_chars_cb)(void* user, uint32_t stream, const char* chars, size_t n);
void hd_set_sentence_callback(hd_engine* e, hd_sentence_cb cb, void* user);   /* fires only on CRC match */
/* every sentence the scan finds, CRC-valid or not, in the order found and before the sentence callback of the same sentence: the point at which
 * the reference prints "<sentence> OK|ERR" and its running tally (Decoder.h:601 -> print_habhub_sentence.cpp:33-62) */
typedef void (*hd_match_cb)(void* user, uint32_t stream, const char* callsign, const char* data, const char* crc, int crc_ok);
void hd_set_match_callback(hd_engine* e, hd_match_cb cb, void* user);
void hd_set_chars_callback(hd_engine* e, hd_chars_cb cb, void* user);         /* printable chars of this call */

/* ---- data path: pushSamples() + operator()() (Decoder.h:206-219, 416-638) for all S streams ----
 * Stream s reads `n` cf32 samples (interleaved I,Q float32: the IQSource_File layout, IQSource_File.h:156-157)
 * starting at `iq + 2*s*stream_stride` floats; stream_stride = 0 makes every stream read the same recording (one recording fanned out to streams
 * tuned to different offsets, hd_stream_set_tune).  `n_per_stream` (S entries) overrides the uniform `n` when not
 * NULL.  Every n must be <= max_chunk and a multiple of the decimation factor (the Decoder facade keeps the
 * remainder queued on the host exactly like Decoder.h:429-435).  Returns after the decoded text of this
 * call has been delivered (callbacks fired, getters updated).  A call the engine refuses (bad sizes, a low-pass design that leaves no taps or exceeds
 * hd_engine_lowpass_taps_max) leaves every stream as it was; a call that fails after its first upload or launch puts the engine into its failed state
 * (HD_ERR_DEVICE from then on). */
int hd_process_host(hd_engine* e, const float* iq, size_t stream_stride, const uint32_t* n_per_stream, uint32_t n);
/* Page-locked host memory the GPU addresses in place.  An IQ buffer that lives in such memory and is handed to hd_process_host of a SYNCHRONOUS engine
 * (pipeline = 0: the call returns when its kernels are done) is read by the first decimation stage straight over PCIe -- no staging copy inside the call
 * (one 65536-sample push of one stream: 512 KiB in ~10 us instead of a ~40 us pageable copy in front of the kernels).  The Decoder facade keeps its input
 * queue (the reference's iq_in_buffer_, Decoder.h:206-219) in it.  NULL when no HIP device is present or the allocation fails: use ordinary memory then. */
void* hd_pinned_alloc(size_t bytes);
void  hd_pinned_free(void* p);
/* Same, but `d_iq` is DEVICE memory on the engine's GPU (HBM-resident batches; base 16-byte aligned,
 * stream_stride even). */
int hd_process_device(hd_engine* e, const void* d_iq, size_t stream_stride, const uint32_t* n_per_stream, uint32_t n);
/* ---- packed IQ: what receivers write (rtl_sdr: cu8, HackRF: cs8, Airspy / SDRplay / most recorders: cs16), expanded on the GPU ----
 * Little-endian, I then Q.  The float a packed sample stands for:
 *     HD_IQ_CS16  4 bytes/sample  (float)v * 2^-15
 *     HD_IQ_CS8   2 bytes/sample  (float)v * 2^-7
 *     HD_IQ_CU8   2 bytes/sample  (float)(2*v - 255) * 2^-8      (centre 127.5: 0 -> -255/256, 255 -> +255/256)
 * Every value is exact in float, so a packed push is, float for float, the cf32 push of hd_host_iq_convert's output (habdec_amd_host.h): a kernel of
 * its own (kernels/iq_unpack.hip) expands the packed rows into the cf32 staging slabs hd_process_host uses, and every kernel behind it runs as on cf32.
 * Only the packed bytes cross the host link: a half (cs16) or a quarter (cs8, cu8) of the cf32 bytes.
 * `stream_stride`, `n_per_stream` and `n` count complex samples as above; a cs16 row may start on any 4-byte boundary and a cs8 / cu8 row on any 2-byte
 * boundary (odd strides, bases with an offset).  HD_IQ_CF32 through these calls IS hd_process_host / hd_process_device, with their alignment rules.
 * Where the bytes come from: pageable host memory, and any host buffer in batch mode, is copied packed into a device slab and unpacked from there;
 * page-locked mapped memory (hd_pinned_alloc) of a synchronous engine is unpacked in place over PCIe (counted in hd_timing.host_calls_in_place); a device
 * pointer is unpacked straight from the caller's buffer.  The call returns when the caller's buffer is theirs again.
 * Errors: an unknown fmt, a null pointer or a base off its sample boundary: HD_ERR_INVALID; n > max_chunk: HD_ERR_CAPACITY; the rest as hd_process_device.
 * A refused call leaves every stream untouched. */
#define HD_IQ_CF32 0
#define HD_IQ_CS16 1
#define HD_IQ_CS8 2
#define HD_IQ_CU8 3
int hd_process_host_fmt(hd_engine* e, int fmt, const void* iq, size_t stream_stride, const uint32_t* n_per_stream, uint32_t n);
int hd_process_device_fmt(hd_engine* e, int fmt, const void* d_iq, size_t stream_stride, const uint32_t* n_per_stream, uint32_t n);
/* Pipelined mode: wait for the call in flight and deliver its results (no-op otherwise).  Getters that read
 * device buffers flush implicitly. */
int hd_flush(hd_engine* e);

/* Batched file ingest: pump `src` (habdec_amd_host.h, hd_host_iqfiles_*; one file per stream, opened
 * with chunk <= max_chunk and granule = the engine's decimation factor) through the engine until the files are exhausted
 * or `max_rounds` rounds were pushed.  A reader thread fills pinned push slabs (four, so that a slab is never refilled
 * while a pipelined call may still copy from it) while the calling thread runs hd_process_host on the previous one --
 * file reads, the H2D copy and the GPU work overlap.  Text is delivered as by hd_process_host; ends with hd_flush.
 * A batch opened with a packed format (hd_host_iqfiles_open_fmt) keeps its slabs packed and goes through hd_process_host_fmt.
 * `samples_done` (optional) receives the IQ samples consumed over all streams. */
struct hd_host_iqfiles;
int hd_ingest_run(hd_engine* e, struct hd_host_iqfiles* src, uint64_t max_rounds, uint64_t* samples_done);

/* ---- results: getRTTY / getLastSentence (Decoder.h:641-652) and the callback streams ---- */
size_t hd_stream_rtty(hd_engine* e, uint32_t stream, char* buf, size_t cap);
size_t hd_stream_last_sentence(hd_engine* e, uint32_t stream, char* buf, size_t cap);
/* drain the log of CRC-valid sentences ("callsign,data*crc\n" each) / of all regex matches / of printable chars */
size_t hd_stream_take_sentences(hd_engine* e, uint32_t stream, char* buf, size_t cap);
size_t hd_stream_take_matches(hd_engine* e, uint32_t stream, char* buf, size_t cap);
size_t hd_stream_take_chars(hd_engine* e, uint32_t stream, char* buf, size_t cap);
uint64_t hd_engine_sentences_ok(const hd_engine* e);   /* CRC-valid sentences over all streams so far */

/* ---- GUI data: getFFT / getDemodulated / getPowerSpectrum / getPeaks / getNoiseFloor / getShift /
 *      getFrequencyCorrection (Decoder.h:751-803) ---- */
typedef struct hd_afc_info {
    double frequency_correction, shift_hz, noise_floor, noise_variance;
    int32_t peak_left, peak_right;      /* sign encodes validity like AFC::getPeaks (AFC.h:146-162) */
    uint64_t spectra;                    /* number of 4096-bin spectra computed so far */
} hd_afc_info;
int    hd_stream_afc(hd_engine* e, uint32_t stream, hd_afc_info* out);
size_t hd_stream_spectrum(hd_engine* e, uint32_t stream, float* iq, size_t cap_complex);   /* freq_out_, fftshifted */
size_t hd_stream_power(hd_engine* e, uint32_t stream, float* p, size_t cap);
size_t hd_stream_demodulated(hd_engine* e, uint32_t stream, float* v, size_t cap);         /* last call */

/* ---- parity taps (not in the reference API; the intermediates its process() holds in members) ---- */
size_t hd_stream_decimated(hd_engine* e, uint32_t stream, float* iq, size_t cap_complex);  /* iq_samples_temp_ of the last call */
size_t hd_stream_filtered(hd_engine* e, uint32_t stream, float* iq, size_t cap_complex);   /* iq_samples_filtered_ (keep_filtered=1) */
size_t hd_stream_bits(hd_engine* e, uint32_t stream, uint8_t* bits, size_t cap);           /* symbols of the last call */
size_t hd_stream_flips(hd_engine* e, uint32_t stream, uint32_t* flips, size_t cap);        /* flip points of the last call */
size_t hd_stream_fir_taps(hd_engine* e, uint32_t stream, float* taps, size_t cap);
uint32_t hd_stream_symbol_backlog(hd_engine* e, uint32_t stream);                          /* samples held by the symbol extractor */
/* Checksum of the discriminator output (getDemodulated(), Decoder.h:131) of the call DELIVERED last for this stream, without flushing the
 * pipeline: ck[0] = sum of the samples' bit patterns, ck[1] = sum of (i + 1) * bit pattern, mod 2^32, over n samples; *call_index counts
 * hd_process_* calls from 0.  Every launch path computes it (n = 0xFFFFFFFF only before the stream's first delivered call). */
int hd_stream_demod_checksum(hd_engine* e, uint32_t stream, uint64_t* call_index, uint32_t* n, uint32_t ck[2]);
/* ... and every call delivered so far folded into one word, so that a free-running batch can be compared with a CPU run call by call without reading a
 * sample: hash = fold over the delivered calls, in order, of (n, ck[0], ck[1]) with h = (h ^ x) * 0x100000001B3 starting from 0xCBF29CE484222325 (FNV-1a over
 * 32-bit words); *calls = calls folded in, *calls_without = delivered calls whose launch path left no checksum (not folded in; 0 since every path fills it). */
int hd_stream_demod_checksum_total(hd_engine* e, uint32_t stream, uint64_t* calls, uint64_t* calls_without, uint64_t* hash);
uint64_t hd_stream_bits_total(hd_engine* e, uint32_t stream);                              /* symbols produced since the engine was created (delivered calls) */
uint64_t hd_stream_flip_list_full(hd_engine* e, uint32_t stream);                          /* delivered calls in which the device's flip list (512 flip points per call) filled up: the symbol search
                                                                                             * stopped there and went on in the next call -- the same bits as SymbolExtractor::operator() (SymbolExtractor.h:129-158,
                                                                                             * which has no such bound), delivered a call later */

/* ---- measurement ---- */
typedef struct hd_timing {
    double ms_total;        /* HIP-event time of the whole kernel sequence of the last hd_process_* call */
    double ms_front;        /* of the kernel that touches full-rate IQ: the first-stage decimator, or the step kernel that contains it (see path) */
    uint64_t front_bytes;   /* algorithmic bytes of that launch: 8 B per input sample + 8 B per output sample */
    uint64_t samples;       /* input samples consumed by the last call over all streams */
    /* host side of the most recent hd_process_* call, microseconds */
    double host_enqueue_us; /* size bookkeeping + uploads + kernel launches */
    double host_wait_us;    /* blocked on the GPU for the results being delivered */
    double host_text_us;    /* AFC state machines, RTTY framing, sentence scan, callbacks */
    uint64_t timed_calls;   /* how many calls carried the HIP-event timing so far (ms_* are those of the latest one) */
    uint32_t path;          /* how the most recent call was launched: 0 separate kernels, 2 stream tail kernel (k_tail), 3 step kernel (k_step:
                             * stage 1 + the previous call's stream tails in one launch; ms_front is ITS duration).  1 (a fused back end) is no longer reported */
    uint32_t step_variant;  /* 1 = the kernel that touches full-rate IQ is one workgroup per CU with LDS-DMA loader waves (stage1_ring.h): k_step_cu on path 3,
                             * k_stage1_cu (stage 1 alone) on paths 0-2; 0 = single-wave / classic workgroups (k_step, k_decimate) */
    uint64_t host_calls_in_place;   /* hd_process_host calls so far whose IQ was read in place from page-locked memory (hd_pinned_alloc): no staging copy */
    uint64_t lowpass_fft_calls;     /* calls so far whose low-pass ran through transforms (fast mode, >= 1024 taps: configs[4]'s 4097-tap filter) */
} hd_timing;
int hd_engine_timing(hd_engine* e, hd_timing* out);
/* Bracket the kernels with HIP events on every `every`-th call (default 8; 0 = never; 1 = every call).  Each event record is
 * a barrier packet that costs a few microseconds of queue time, so per-call timing slows a pipelined batch by ~8 %;
 * hd_engine_timing() reports the most recent timed call. */
void hd_engine_set_timing(hd_engine* e, int every);

/* ---- wideband survey: where in a capture are the payloads? (not in the reference: its only spectrum is per decoder, at the decimated rate) ----
 * A Welch-averaged power spectrum of cf32 IQ at the INPUT rate, and a detector on top of it whose candidate offsets are what hd_stream_set_front_tune
 * takes, sign included: survey (one bin = fs / 4096) -> front tune -> the per-stream AFC / hd_stream_set_auto_afc for the fine part.
 *  - Segments: a push of n samples contributes n < 4096 ? 0 : 1 + (n - 4096) / 2048 segments; segment s is samples [2048 s, 2048 s + 4096) of THAT push.
 *    Segments never straddle pushes and the samples behind the last whole hop are not used: push a capture in large pieces.
 *  - Per segment: periodic Hann window (hd_host_survey_window: a float table, one rounded multiply per part), the engine's 4096-point in-wave transform,
 *    re^2 + im^2 per bin.  One wave sums a run of r = min(HD_SURVEY_RUN, ceil(segments / runs_per_launch)) consecutive segments in float (runs_per_launch =
 *    1024; environment HD_SURVEY_RUNS, read by hd_survey_create); the runs' rows are added in run order into double accumulators that live as long as
 *    the survey.  No floating-point atomics: the same pushes give the same bytes, from device or from host memory.
 *  - Queue: the survey's launches and copies run on a HIP stream of its own.  It never waits for, drains or reorders the engine's pipeline
 *    (hd_survey_destroy frees device memory, which waits for the device).  A survey uses its engine's device, sampling rate, twiddles and mutex: destroy
 *    it before the engine.  Calls are serialised by the engine's mutex, like the getters.
 *  - Errors: null arguments and a device pointer that is not 8-byte aligned are HD_ERR_INVALID; an engine in its failed state is HD_ERR_DEVICE. */
#define HD_SURVEY_BINS 4096
#define HD_SURVEY_HOP 2048
#define HD_SURVEY_RUN 64
typedef struct hd_survey hd_survey;
int  hd_survey_create(hd_engine* e, hd_survey** out);
void hd_survey_destroy(hd_survey* sv);
int  hd_survey_reset(hd_survey* sv);                       /* accumulators = 0, segments = 0 */
/* n cf32 samples in DEVICE memory on the engine's GPU (or page-locked mapped host memory by its device address), 8-byte aligned.  Returns once the
 * launches are queued: the buffer must stay valid until hd_survey_power / hd_survey_detect / hd_survey_reset has returned.  n < 4096: HD_OK, adds nothing. */
int  hd_survey_push_device(hd_survey* sv, const void* d_iq, uint64_t n);
/* The same from host memory, pageable or page-locked, staged through a device slab in pieces of whole runs -- segmentation and run structure are those
 * of the one push, so the result is byte-identical to hd_survey_push_device of the same samples.  The buffer is the caller's again on return. */
int  hd_survey_push_host(hd_survey* sv, const float* iq, uint64_t n);
/* The same pushes of packed IQ (HD_IQ_*; n in complex samples): host and device pushes alike go through the 4 MiB slab loop of hd_survey_push_host on the
 * survey's queue, each slab's whole runs unpacked into it in front of the transform -- byte-identical to hd_survey_push_host of the converted floats.
 * Both return when the buffer is the caller's again.  HD_IQ_CF32 is the plain call; an unknown fmt or a base off its sample boundary: HD_ERR_INVALID. */
int  hd_survey_push_host_fmt(hd_survey* sv, int fmt, const void* iq, uint64_t n);
int  hd_survey_push_device_fmt(hd_survey* sv, int fmt, const void* d_iq, uint64_t n);
/* Waits for the survey's own queue only.  p[i] = acc[i] / (segments * sum w^2) (the sum in double over the float table) belongs to
 * f = (i - 2048) fs / 4096: white noise of complex variance s^2 reads about s^2.  No segments yet: zeros.  Returns the bins written (4096), 0 when
 * cap < 4096 (nothing written), or a negative HD_ERR_*; *segments (optional) = segments accumulated since creation or the last reset. */
int  hd_survey_power(hd_survey* sv, double* p, size_t cap, uint64_t* segments);
typedef struct hd_survey_params {
    double threshold_db;   /* a bin is marked at P >= floor * max(10^(threshold_db / 10), 1 + 8 / sqrt(segments)); default 6 */
    double merge_hz;       /* marked bins with at most ceil(merge_hz / (fs / 4096)) unmarked bins between them form one cluster; default 1500 */
    double dc_guard_hz;    /* > 0: bins with |f| < dc_guard_hz count neither for the floor nor as candidates (a receiver's DC spike); default 0 */
    double max_width_hz;   /* > 0: clusters wider than this are dropped (broadcast carriers, not RTTY); default 0 */
} hd_survey_params;
typedef struct hd_survey_candidate {
    double offset_hz;      /* power-weighted centroid of the cluster's marked bins: what hd_stream_set_front_tune takes */
    double snr_db;         /* 10 log10(sum (P_i - floor) / floor) over the marked bins */
    double width_hz;       /* (bin_hi - bin_lo + 1) fs / 4096 */
    uint32_t bin_lo, bin_hi;
} hd_survey_candidate;
void hd_survey_params_default(hd_survey_params* p);
/* hd_survey_power followed by hd_host_survey_detect (habdec_amd_host.h has the algorithm).  *found = clusters found, the first min(found, cap) of them
 * are written, strongest first.  Fewer than 16 segments: HD_ERR_UNSUPPORTED. */
int  hd_survey_detect(hd_survey* sv, const hd_survey_params* p, hd_survey_candidate* out, uint32_t cap, uint32_t* found);

/* ---- waterfall: WHEN does a payload transmit? (not in the reference) ----
 * The survey sums a whole capture into one spectrum; the waterfall keeps the float rows the survey's kernel forms per run of segments, runs the survey's
 * marking rule on every row on the GPU, counts hits per bin there, and links the marks into tracks on the host: offset_hz (what
 * hd_stream_set_front_tune takes), first_sample and end_sample (when to hd_baud_probe_reset a stream, and when a stream is free again).
 *  - Segments: the survey's.  A push of n samples has n < 4096 ? 0 : 1 + (n - 4096) / 2048 segments; segment s is samples [2048 s, 2048 s + 4096) of THAT
 *    push.  Segments never straddle pushes.  A push shorter than 4096 samples adds no row, but its samples still count towards first_sample of later rows.
 *  - Rows: with L = slot_segments, row j of a push is the float sum, in segment order, of re^2 + im^2 per bin over segments [j L, min((j + 1) L, n_seg)) --
 *    per segment the survey's window, in-wave transform and fftshifted store: exactly what one wave of the survey's kernel produces for a run of L.
 *    first_sample = samples pushed before this push + 2048 j L.  The last row of a push may hold fewer than L segments; below 16 it is flagged
 *    HD_WF_SHORT.  Rows are raw sums: divide by segments * sum w^2 (hd_host_survey_window) for the survey's scale.  So push pieces of
 *    4096 + (k L - 1) * 2048 samples (k whole rows and no sample unused), or much larger ones.
 *  - Detector, per row, on the GPU, all in float, every operation rounded once (hd_host_waterfall_detect_row is the same in plain C++):
 *     1. If any of the 4096 bins has a bit pattern above 0x7F800000 (a NaN or a set sign bit) the row is HD_WF_BAD.
 *     2. Eligible bins: those with |f_i| >= dc_guard_hz, f_i = (i - 2048) fs / 4096.  A guard that leaves no bin: hd_waterfall_create is HD_ERR_INVALID.
 *     3. floor = the median of the m eligible values: s[m / 2] for m odd, 0.5f * (s[m / 2 - 1] + s[m / 2]) for m even, s in ascending order (for the
 *        patterns step 1 admits, the order of the patterns read as unsigned integers).  floor == 0 or floor == +inf: the row is HD_WF_NO_FLOOR.
 *     4. level = floor * F[segments], F[s] = (float)max(10^(threshold_db / 10), 1 + 8 / sqrt(s)), computed in double on the host.
 *     5. Bit i & 31 of word i >> 5 is set when bin i is eligible and row[i] >= level; n_marked is the popcount.
 *     6. A flagged row has no marks and does not count for hits.  floor and level are 0 in a BAD or NO_FLOOR row; a row that is only SHORT has both.
 *  - Hits: hits[i] = the unflagged rows since creation or reset in which bin i is marked, counted on the GPU in integers; rows_counted = those rows.
 *  - Tracks (hd_host_waterfall_tracks is the function; g = ceil(merge_hz / (fs / 4096)) as in the survey):
 *     1. Rows are processed in order; a flagged row is a row without marks.
 *     2. A row's clusters are the survey's: runs of marked bins with at most g unmarked bins between neighbours, no wrap-around; each carries
 *        (lo, hi, n, sum of indices).
 *     3. In ascending lo, a cluster joins the first open track, in order of creation, with lo <= t.hi + g && hi + g >= t.lo (t.lo, t.hi: the track's
 *        cumulative range, which the cluster widens); a cluster that joins none opens a track.
 *     4. After row r a track with r - last_row > gap_rows is closed.
 *    Tracks with rows_hit < min_rows, or wider than max_width_hz when that is > 0, are dropped; the rest come ordered by first_sample, then offset_hz.
 *    *found = tracks, the first min(found, cap) are written.
 *  - Queue and lifetime: like the survey -- a HIP stream of its own, the engine's device, sampling rate, twiddles and mutex; it never waits for, drains or
 *    reorders the engine's pipeline; destroy it before the engine.  Every push returns when the caller's buffer is theirs again and the new rows' headers
 *    and marks are in host memory (528 bytes per row read back on the waterfall's queue).  A push is worked off in launches of at most 1024 rows (environment
 *    HD_WATERFALL_CHUNK, read by hd_waterfall_create; rows, headers and marks do not depend on it), cut also where the ring wraps.  The float rows stay in a device ring of rows_cap rows;
 *    headers and marks of all rows since creation or reset are kept on the host.
 *  - Same rows from every source: host and packed pushes go through a staging slab that carries whole rows; rows, headers and marks are byte-identical
 *    to one hd_waterfall_push_device of the same samples (packed: of hd_host_iq_convert's floats).
 *  - hd_waterfall_push_rows: n_rows rows of 4096 float sums made elsewhere, of segments[r] segments each (1..64; a host array), from host (device = 0) or
 *    device memory (4-byte aligned); they are copied into the ring and go through the same detector.  Row r's first_sample is the sample count so
 *    far, which the row advances by 2048 segments[r].
 *  - Errors: null arguments, slot_segments outside 16..64, rows_cap == 0, negative or NaN parameters, a cf32 base off 8 bytes or a packed base off its
 *    sample boundary, a pointer that is not device memory where one is wanted, segments[r] outside 1..64, rows outside the kept range are
 *    HD_ERR_INVALID; an engine in its failed state is HD_ERR_DEVICE. */
#define HD_WATERFALL_WORDS 128          /* 4096 mark bits per row */
#define HD_WF_SHORT    1u               /* fewer than 16 segments: no marks */
#define HD_WF_BAD      2u               /* some bin of the row is NaN or has its sign bit set: no marks */
#define HD_WF_NO_FLOOR 4u               /* floor == 0 or floor == +inf: no marks */
typedef struct hd_waterfall hd_waterfall;
typedef struct hd_waterfall_params {
    uint32_t slot_segments;   /* L: segments summed per row, 16..64; default 16 */
    uint32_t rows_cap;        /* float rows kept on the device (a ring), >= 1; default 1024 (16 MiB) */
    double   threshold_db;    /* as hd_survey_params; default 6 */
    double   dc_guard_hz;     /* as hd_survey_params; default 0 */
} hd_waterfall_params;
typedef struct hd_waterfall_row {       /* 32 bytes */
    uint64_t first_sample;    /* absolute index, since creation / reset, of the row's first sample */
    uint32_t segments;        /* 1..L */
    uint32_t flags;           /* HD_WF_* */
    float    floor, level;    /* 0 where the flags leave them undefined */
    uint32_t n_marked, _pad;
} hd_waterfall_row;
typedef struct hd_waterfall_track_params {
    double   merge_hz;        /* as hd_survey_params, within a row and between a cluster and a track; default 1500 */
    double   max_width_hz;    /* > 0: tracks wider than this are dropped; default 0 */
    uint32_t gap_rows;        /* a track survives this many rows without a mark; default 1 */
    uint32_t min_rows;        /* tracks marked in fewer rows are dropped; default 3 */
} hd_waterfall_track_params;
typedef struct hd_waterfall_track {     /* 72 bytes */
    uint64_t first_sample;    /* first_sample of first_row */
    uint64_t end_sample;      /* first_sample of last_row + (segments of last_row + 1) * 2048: one past the last sample of the last marked row */
    uint64_t first_row, last_row;
    uint64_t marks;           /* marked bins over all its rows */
    double   offset_hz;       /* (sum of marked indices / marks - 2048) fs / 4096: what hd_stream_set_front_tune takes */
    double   width_hz;        /* (bin_hi - bin_lo + 1) fs / 4096 */
    uint32_t rows_hit;        /* distinct rows with a mark of the track */
    uint32_t bin_lo, bin_hi;  /* cumulative range */
    int32_t  open;            /* 1: still open after the last row (the payload may be going on) */
} hd_waterfall_track;
void hd_waterfall_params_default(hd_waterfall_params* p);
void hd_waterfall_track_params_default(hd_waterfall_track_params* p);
int  hd_waterfall_create(hd_engine* e, const hd_waterfall_params* p /* null: defaults */, hd_waterfall** out);
void hd_waterfall_destroy(hd_waterfall* wf);
int  hd_waterfall_reset(hd_waterfall* wf);                 /* rows, hits and the sample count = 0 */
/* n cf32 samples in device memory (as hd_survey_push_device) / in host memory; packed IQ (HD_IQ_*) from either.  All four return when the buffer is the
 * caller's again and the push's headers and marks are in host memory. */
int  hd_waterfall_push_device(hd_waterfall* wf, const void* d_iq, uint64_t n);
int  hd_waterfall_push_host(hd_waterfall* wf, const float* iq, uint64_t n);
int  hd_waterfall_push_device_fmt(hd_waterfall* wf, int fmt, const void* d_iq, uint64_t n);
int  hd_waterfall_push_host_fmt(hd_waterfall* wf, int fmt, const void* iq, uint64_t n);
/* rows of float sums made elsewhere (and the detector's test door): n_rows rows of 4096 floats, segments[r] each, host or device memory */
int  hd_waterfall_push_rows(hd_waterfall* wf, const float* rows, const uint32_t* segments, uint32_t n_rows, int device);
uint64_t hd_waterfall_rows_total(hd_waterfall* wf);        /* rows since creation or reset (0 for a null waterfall) */
/* rows [first_row, first_row + n) must exist (n may be 0) */
int  hd_waterfall_headers(hd_waterfall* wf, uint64_t first_row, uint32_t n, hd_waterfall_row* out);
int  hd_waterfall_marks(hd_waterfall* wf, uint64_t first_row, uint32_t n, uint32_t* out /* n * 128 words */);
int  hd_waterfall_rows(hd_waterfall* wf, uint64_t first_row, uint32_t n, float* out /* n * 4096 */);   /* only rows still in the ring, else HD_ERR_INVALID */
int  hd_waterfall_hits(hd_waterfall* wf, uint32_t hits[4096], uint64_t* rows_counted);
int  hd_waterfall_tracks(hd_waterfall* wf, const hd_waterfall_track_params* p /* null: defaults */, hd_waterfall_track* out, uint32_t cap, uint32_t* found);

/* ---- baud-rate probe: what is a stream's symbol rate? (not in the reference, which is told it: Decoder::baud()) ----
 * survey -> front tune -> AFC -> PROBE -> hd_stream_set_baud -> framing trial (below) -> hd_stream_set_rtty.  A probe is attached to an engine like a
 * survey (its device and mutex; destroy it before the engine) and accumulates, per stream, integer statistics of the discriminator output
 * (hd_stream_demodulated) over as many calls as are pushed; an estimate is read from them on the host.  fsd = hd_engine_decimated_rate(e).
 *  - Candidates: HD_PROBE_CANDIDATES of them, b_k = baud_lo (baud_hi / baud_lo)^(k / 1023) in double, F_k = (uint64)floor(b_k / fsd 2^32 + 0.5).
 *    hd_baud_probe_create is HD_ERR_INVALID unless 0 < baud_lo < baud_hi <= fsd / 3.5 (and min_coherence >= 0).
 *  - Sign bits: b[i] = d[i] > 0.0f (NaN gives 0), b[j] = 0 in front of the stream's first sample since the last reset; i = the stream's absolute sample
 *    index since the last reset, uint64.
 *  - Scales: W in {1, 3, 7, 15, 31, 63, 127, 255, 511}; m_W[i] = popcount(b[i-W+1 .. i]) > (W-1)/2; an edge of scale W stands at i when i >= W and
 *    m_W[i] != m_W[i-1].  Candidate k listens to the largest W <= max(1, T_k / 4), T_k = 2^32 / F_k in double.
 *  - Per edge and candidate: p = i F_k mod 2^64, idx = (p >> 22) & 1023, block = (uint32)(p >> 38) (the group of 64 candidate periods the edge falls
 *    into).  block != cur_block_k: the block is dumped and cur_block_k = block.  Then n_k += 1 and, while n_k <= 4096, re_k += C[idx],
 *    im_k += C[(idx + 768) & 1023], C[a] = (int32)nearbyint(32767 cos(2 pi a / 1024)).
 *  - Dump: if 8 <= n_k <= 4096 then P_k += re_k^2 + im_k^2, Q_k += n_k^2, NB_k += 1; then re_k = im_k = n_k = 0.
 *  - Estimate (host, double; on a copy of the state whose open blocks are dumped by the same rule): rho_k = NB_k >= 4 ? P_k / (32767^2 Q_k) : 0 -- 1 when
 *    every edge of every block sits at one phase of the candidate's period, about 1 / n for random edges.  settled = ((i F_0) >> 38) >= 4: four whole
 *    blocks of the lowest candidate, 6.4 s at baud_lo = 40.  valid = settled && rho_max >= min_coherence.  k* = the lowest k with rho_k >= rho_max / 2,
 *    moved up while rho_{k+1} > rho_k (the baud line and its harmonics all read about 1: the fundamental is the lowest; sub-harmonics at the character
 *    rate are coherent for the start-bit edges only).  baud = the vertex of the parabola through (ln b, rho) at k*-1, k*, k*+1, clamped to
 *    [b_{k*-1}, b_{k*+1}]; b_{k*} at the grid's ends.  nominal = the entry of {45.45, 50, 75, 100, 110, 134.5, 150, 200, 300, 600, 1200} nearest in
 *    ratio if within 1.5 %, else 0.
 *  - A stream that repeats one sparse character is periodic at its character rate, and the answer may be that rate.
 *  - Queue: launches run on the engine's first queue; every push returns when its kernel is done.  Calls are serialised by the engine's mutex.
 *  - Errors: null arguments and bad parameters are HD_ERR_INVALID; an engine in its failed state is HD_ERR_DEVICE. */
#define HD_PROBE_CANDIDATES 1024
#define HD_PROBE_SCALES 9
typedef struct hd_baud_probe hd_baud_probe;
typedef struct hd_baud_probe_params {
    double baud_lo, baud_hi;   /* the candidate grid's ends; defaults 40 and 1300 */
    double min_coherence;      /* an estimate is valid at rho_max >= this; default 0.5 */
} hd_baud_probe_params;
typedef struct hd_baud_estimate {
    double baud, nominal;      /* nominal = 0: no standard rate within 1.5 % */
    double rho, rho_max;       /* coherence of candidate k, and the largest of all candidates */
    uint64_t samples;          /* i: samples pushed since the last reset */
    uint64_t edges;            /* edges of the scale candidate k listens to */
    uint32_t k;                /* k* */
    int32_t  settled, valid;
    uint32_t _pad;
} hd_baud_estimate;
/* The raw accumulators (parity tests).  history: bit (j & 63) of word ((j >> 6) & 7) is the sign bit of the newest sample j' < i with j' = j mod 512. */
typedef struct hd_baud_probe_stream_state {
    uint64_t samples;                       /* i */
    uint64_t edges[HD_PROBE_SCALES];        /* edges seen per scale */
    uint64_t history[8];
    uint32_t majority[HD_PROBE_SCALES];     /* m_W[i-1] per scale */
    uint32_t n_candidates;                  /* HD_PROBE_CANDIDATES */
} hd_baud_probe_stream_state;
typedef struct hd_baud_probe_candidate {
    uint64_t P, Q;
    uint32_t NB;
    int32_t  re, im;
    uint32_t n, cur_block, _pad;
} hd_baud_probe_candidate;
void hd_baud_probe_params_default(hd_baud_probe_params* p);
int  hd_baud_probe_create(hd_engine* e, const hd_baud_probe_params* p /* null: the defaults */, hd_baud_probe** out);
void hd_baud_probe_destroy(hd_baud_probe* p);
int  hd_baud_probe_reset(hd_baud_probe* p, uint32_t stream /* UINT32_MAX: all */);
/* Adds, for every stream, the discriminator output of the call delivered last (what hd_stream_demodulated returns), read where the call left it: one
 * launch for all streams behind a drain of the pipeline, like the data getters (not from inside a callback).  A call that was pushed already, and a
 * stream whose call produced no output, add nothing: HD_OK. */
int  hd_baud_probe_push_engine(hd_baud_probe* p);
/* Rows of any discriminator output: stream s adds n_per_stream[s] (null: n) floats at rows + s * stride, from device memory on the engine's GPU (4-byte
 * aligned) or from host memory.  The buffer is the caller's again on return. */
int  hd_baud_probe_push_device(hd_baud_probe* p, const float* d_rows, size_t stride, const uint32_t* n_per_stream, uint32_t n);
int  hd_baud_probe_push_host(hd_baud_probe* p, const float* rows, size_t stride, const uint32_t* n_per_stream, uint32_t n);
/* A copy of the stream's state followed by hd_host_baud_probe's estimate (habdec_amd_host.h). */
int  hd_baud_probe_estimate(hd_baud_probe* p, uint32_t stream, hd_baud_estimate* out);
/* Returns HD_PROBE_CANDIDATES; *hdr (optional) is written, and the candidates when cap >= HD_PROBE_CANDIDATES -- with a smaller cap nothing at all is
 * written.  Negative: HD_ERR_*. */
int  hd_baud_probe_state(hd_baud_probe* p, uint32_t stream, hd_baud_probe_stream_state* hdr, hd_baud_probe_candidate* candidates, size_t cap);

/* ---- framing trial: 7 or 8 data bits, 1 or 2 stop bits? (not in the reference) ----
 * Once the baud rate is set the bits flow; while a stream's trial is on, the bits delivered for it are also pushed into four text stages (7N1, 7N2, 8N1,
 * 8N2: formats 0..3) beside its own, in every pipeline mode.  The stream's own text stage, callbacks and getters are untouched.  Turning the trial on
 * resets it; turning it off drops it.  best = -1 while no format has a CRC-valid sentence; else, among the formats whose sentences_ok is the largest,
 * the one with the most stop bits, then the most data bits (a one-stop framer also frames a two-stop signal: the stricter format that loses nothing). */
#define HD_TRIAL_FORMATS 4
typedef struct hd_format_trial_result {
    int32_t  best;                 /* format index or -1 */
    uint32_t best_bits;            /* what hd_stream_set_rtty takes (0 when best = -1) */
    float    best_stops;
    uint32_t bits[HD_TRIAL_FORMATS];
    float    stops[HD_TRIAL_FORMATS];
    uint32_t _pad;
    uint64_t sentences_ok[HD_TRIAL_FORMATS], matches[HD_TRIAL_FORMATS], printable[HD_TRIAL_FORMATS];
} hd_format_trial_result;
int hd_stream_set_format_trial(hd_engine* e, uint32_t stream, int on);
int hd_stream_format_trial(hd_engine* e, uint32_t stream, hd_format_trial_result* out);   /* HD_ERR_INVALID while the trial is off */

/* ---- clocked soft-decision decoder with CRC-guided repair: for weak signals (not in the reference) ----
 * probe -> hd_stream_set_baud -> trial -> hd_stream_set_rtty -> hd_clocked_set_modem.  The engine's own chain (flip points of quarter-bit means, run
 * lengths rounded to bits, a framer hunting for start and stop bits) is the reference's and stays; a discriminator click costs it a bit and with the bit
 * the character alignment of a sentence.  A clocked decoder is attached to an engine like a probe and reads the same rows (hd_stream_demodulated).  Per
 * stream it starts a bit clock at every start edge, takes one decision per bit from the sum over the whole bit, and keeps the sums as soft values; a
 * host stage runs the sentence scan and CRC of the ordinary text stage over the characters and, where a match's CRC fails, flips the least confident
 * bits.  All of it is integer arithmetic: kernel, host restatement (hd_host_clocked_*) and a numpy model agree bit for bit.
 *  - Indices are absolute sample indices of a stream since its last reset (uint64); how a stream is cut into pushes cannot matter.
 *  - Quantised sample: q_i = 0 for NaN, else (int32)(clamp(v_i, -4, 4) * 1024) truncated toward zero; negated when the stream's `invert` is set (tones
 *    swapped).  S(a, b) = the exact sum of q_i, a <= i < b.
 *  - Clock: F = (int64)floor(fsd / baud * 65536 + 0.5); full = (F + 32768) >> 16; h = max(2, (F + 65536) >> 17); bit boundary k of a character whose
 *    start edge is x: B_k = x + ((k F + 32768) >> 16).  K = 1 + nbits + nstops bits per character; look = h + ((K F + 32768) >> 16).
 *    hd_clocked_set_modem is HD_ERR_UNSUPPORTED unless 3.5 <= fsd / baud <= HD_CLOCKED_MAX_SPB (2048), nbits is 7 or 8 and nstops 1 or 2.
 *  - Scan: the cursor p starts at h.  Position p is decided once p + look <= n, n = samples pushed -- every sample any decision at p can read exists
 *    then; else the stream waits for the next push.  (One rule for every kind of decision: the state after n samples is a function of those samples.)
 *    Edge test at p: S(p-h, p) > 0 && S(p, p+h) < 0.  False: p += 1.  True: x = the smallest x in [p, p+h] that minimises S(x, x+full) - S(x-h, x);
 *    start = S(B_0, B_1), data_k = S(B_{1+k}, B_{2+k}) for k < nbits, stop = S(B_{1+nbits}, B_{2+nbits}), stop2 = S(B_{2+nbits}, B_{3+nbits}) with two
 *    stop bits (else 0; recorded, no condition).  Accepted iff start < 0 && stop > 0: a record {pos = x, ch = sum over k of (data_k > 0) << k, data,
 *    start, stop, stop2} is appended, characters += 1 and p = x + (((2 (1 + nbits) + 1) F + 65536) >> 17), the middle of the first stop bit.
 *    Rejected: rejects += 1, p += 1.
 *  - Records lie in a per-stream ring of record_cap entries on the GPU until hd_clocked_records or hd_clocked_take_sentences takes them; a record
 *    appended to a full ring overwrites the oldest untaken one, dropped += 1.
 *  - Text (host; what the engine's text stage does behind its framer): characters 32..126 and '\n' are appended to the stream's text with their
 *    records; while the text is longer than 20 characters the sentence scan runs; a match with the right CRC16 is a plain sentence (flips = 0); the
 *    text is cut as the text stage cuts it (4 characters behind the terminator; above 1000 characters at the last '$').
 *  - Repair, for a match whose CRC fails (matches_failed += 1): the span is the match from its first '$' to the CRC's last character.  The repair_bits
 *    (default 8) data bits of the span with the smallest |data_k| -- ties: the earlier character, then the lower bit -- are the list; all subsets of size
 *    1, then 2, ... up to repair_flips (default 3) are tried in the list's lexicographic order (92 trials).  A trial flips its bits (ch bit k of the
 *    character); it counts if every character it changed is in 32..126 afterwards, the sentence scan on the changed span alone matches the whole span
 *    (from its first character to its last) and the CRC16 agrees.  The first trial that counts wins: a repaired sentence with flips = the subset's
 *    size.  Either limit 0: no repair.
 *  - False accepts: a trial on a span that is not the transmitted sentence passes the CRC16 with probability 2^-16, so a failed match yields a
 *    sentence that was not sent with probability at most 92 * 2^-16 = 0.14 % at the default limits, before the printable and shape filters.
 *  - Sentences, plain and repaired, leave through hd_clocked_take_sentences only: never through hd_set_sentence_callback, hd_engine_sentences_ok or
 *    any getter of the engine.
 *  - Queue, errors: as the probe's.  One launch per push for all streams (a push of more than HD_CLOCKED_CHUNK samples for a stream: one launch per
 *    chunk); every push returns when its kernels are done. */
#define HD_CLOCKED_MAX_SPB 2048
#define HD_CLOCKED_RING 32768      /* per-stream sample history on the GPU, kept as running sums */
#define HD_CLOCKED_CHUNK 4096      /* samples per stream and launch */
typedef struct hd_clocked hd_clocked;
typedef struct hd_clocked_params {
    uint32_t record_cap;       /* records per stream the ring holds; default 4096, at least 16 */
    uint32_t repair_bits;      /* default 8, at most 16 */
    uint32_t repair_flips;     /* default 3, at most 4 */
    uint32_t _pad;
} hd_clocked_params;
typedef struct hd_clocked_record {
    uint64_t pos;              /* x */
    int32_t  data[8];          /* data_k; data[7] = 0 with 7 data bits */
    int32_t  start, stop, stop2;
    uint32_t ch;
} hd_clocked_record;
typedef struct hd_clocked_sentence {
    uint64_t pos;              /* pos of the record of the sentence's first '$' */
    uint32_t flips;            /* 0: plain */
    uint32_t len;              /* strlen of callsign,data*CRC (text holds at most 495 characters of it, NUL-terminated) */
    char     text[496];
} hd_clocked_sentence;
typedef struct hd_clocked_counters {
    uint64_t samples, cursor;  /* n and p */
    uint64_t characters, rejects, dropped;
    uint64_t matches_failed, sentences_plain, sentences_repaired;
} hd_clocked_counters;
void hd_clocked_params_default(hd_clocked_params* p);
/* Every stream takes the engine stream's current baud rate and framing; a stream whose settings hd_clocked_set_modem would refuse is off (pushes pass
 * it by) until it is given a modem. */
int  hd_clocked_create(hd_engine* e, const hd_clocked_params* p /* null: the defaults */, hd_clocked** out);
void hd_clocked_destroy(hd_clocked* c);
/* Samples, cursor, records, text and counters of the stream start again; sentences not yet taken stay. */
int  hd_clocked_reset(hd_clocked* c, uint32_t stream /* UINT32_MAX: all */);
int  hd_clocked_set_modem(hd_clocked* c, uint32_t stream, double baud, uint32_t nbits, uint32_t nstops, int invert);   /* resets the stream */
/* The three routes of the probe, with its rules (hd_baud_probe_push_*). */
int  hd_clocked_push_engine(hd_clocked* c);
int  hd_clocked_push_device(hd_clocked* c, const float* d_rows, size_t stride, const uint32_t* n_per_stream, uint32_t n);
int  hd_clocked_push_host(hd_clocked* c, const float* rows, size_t stride, const uint32_t* n_per_stream, uint32_t n);
/* Takes up to cap of the stream's oldest untaken records off the ring (they pass through the text stage on their way) and returns how many were
 * written; out null: takes none and returns how many wait.  Negative: HD_ERR_*. */
int  hd_clocked_records(hd_clocked* c, uint32_t stream, hd_clocked_record* out, size_t cap);
/* Takes all waiting records into the text stage, then hands out up to cap of the stream's sentences, oldest first; returns how many were written. */
int  hd_clocked_take_sentences(hd_clocked* c, uint32_t stream, hd_clocked_sentence* out, size_t cap);
int  hd_clocked_stats(hd_clocked* c, uint32_t stream, hd_clocked_counters* out);

/* ---- tone-filter demodulator: a row for the clocked decoder and the probe below the discriminator's threshold (not in the reference) ----
 * probe -> trial -> TONES -> hd_clocked_push_device.  The polar discriminator (hd_stream_demodulated) differentiates phase; once the noise makes the phase
 * jump, its row carries nothing for any decoder.  The receiver for that level correlates the IQ against the two tones over about a bit and compares the
 * envelopes: noncoherent FSK detection, mark and space filters.  A tones object is attached to an engine like a probe (its device, mutex and first queue;
 * destroy it before the engine), reads each stream's tuned decimated IQ (hd_stream_decimated) and writes one float row per stream in device memory, which
 * hd_clocked_push_device and hd_baud_probe_push_device take as they take any row.  Integer arithmetic behind the quantisation: kernel, host restatement
 * (hd_host_tones_*) and a numpy model agree byte for byte.  fsd = hd_engine_decimated_rate(e).
 *  - Modem of a stream: baud, the upper and the lower tone f_hi, f_lo in Hz at the decimated rate, and the object's window_q8.
 *    F = (int64)floor(fsd / baud * 65536 + 0.5), full = (F + 32768) >> 16 (the clocked decoder's F and full), W = max(1, (F window_q8 + 2^23) >> 24),
 *    L = 8 full, Phi_t = (uint32)(int64)nearbyint(f_t / fsd * 2^32), ties to even.  hd_tones_set_modem is HD_ERR_UNSUPPORTED unless
 *    3.5 <= fsd / baud <= HD_TONES_MAX_SPB (2048) and 32 <= window_q8 <= 256, HD_ERR_INVALID for |f_t| >= fsd / 2 or an f_hi that is not above f_lo.
 *  - i = the stream's absolute sample index since its last reset, uint64; how a stream is cut into pushes cannot matter; samples in front of index 0
 *    are zero.
 *  - Quantise, per component of the cf32 sample: q = 0 for NaN, else (int32)(clamp(v, -8, 8) * 256) truncated toward zero.
 *  - Rotate, per tone t: theta = (i Phi_t) mod 2^32, a = theta >> 22, c = C[a], s = C[(a + 768) & 1023], C[a] = (int32)nearbyint(32767 cos(2 pi a / 1024))
 *    (the probe's table); r_re = (q_re c + q_im s) >> 15, r_im = (q_im c - q_re s) >> 15, arithmetic shifts (floor).
 *  - Window: s_re(i) = the sum of r_re(j), max(0, i + 1 - W) <= j <= i, s_im likewise.  Envelope: A_t(i) = floor(sqrt(s_re^2 + s_im^2)), the exact integer
 *    root.
 *  - Normaliser: T(i) = A_hi(i) + A_lo(i); N(i) = the sum of T(j), max(0, i + 1 - L) <= j <= i.
 *  - Output: o = ((A_hi - A_lo) * 1024 * L) / max(1, N), int64 division truncated toward zero, clamped to [-4096, 4096]; the float written is o / 1024.0f,
 *    exact, and the clocked decoder's quantisation of it gives back o.  Positive means the upper tone, the discriminator's sign: `invert` of
 *    hd_clocked_set_modem means the same with either row.
 *  - After hd_tones_create no stream has a modem: a stream without one is passed by and its row has length 0.  Every stream remembers the engine stream's
 *    baud rate of that moment; baud = 0 in hd_tones_set_modem stands for it.
 *  - The tones: the AFC's peaks (hd_stream_afc) are unreliable at the levels this object is for -- at sigma 1.1 on the 300 baud signal of NOTES.md the
 *    reference's AFC reports peaks 420 Hz and 74 Hz off.  Take the tones while the signal is strong (hd_tones_set_modem_from_afc), or from the nominal
 *    shift around a known centre.  A payload that was never strong has its tones found by the tone search below (hd_tone_search_*), whose result is
 *    what hd_tones_set_modem takes.
 *  - Queue, errors: as the probe's.  One launch for all streams per HD_TONES_CHUNK samples of the longest row; every push returns when its kernels are
 *    done.  A push of more than max_push samples for a stream is HD_ERR_CAPACITY. */
#define HD_TONES_MAX_SPB 2048
#define HD_TONES_CHUNK 4096        /* samples per stream and launch */
typedef struct hd_tones hd_tones;
typedef struct hd_tones_params {
    uint32_t max_push;         /* samples per stream and push the rows hold; default (0): the engine's largest decimated chunk per call, at least 4096 */
    uint32_t window_q8;        /* the tone filters' length in 1/256 bit; default 160, 32 .. 256 */
} hd_tones_params;
typedef struct hd_tones_info {
    uint64_t samples;          /* i: samples pushed since the last reset */
    uint32_t F, full, W, L;    /* F = 0: the stream has no modem */
    uint32_t step_hi, step_lo; /* Phi_hi, Phi_lo */
} hd_tones_info;
void hd_tones_params_default(hd_tones_params* p);
int  hd_tones_create(hd_engine* e, const hd_tones_params* p /* null: the defaults */, hd_tones** out);   /* HD_ERR_UNSUPPORTED: window_q8 */
void hd_tones_destroy(hd_tones* t);
int  hd_tones_reset(hd_tones* t, uint32_t stream /* UINT32_MAX: all */);     /* the sample index starts again; the modem stays; the rows have length 0 */
int  hd_tones_set_modem(hd_tones* t, uint32_t stream, double baud, double f_hi_hz, double f_lo_hz);       /* resets the stream */
/* The tones from the stream's AFC: tone = (peak bin - 2048) * fsd / 4096 of hd_afc_info's peak_right and peak_left.  HD_ERR_INVALID unless both peaks
 * are valid (positive). */
int  hd_tones_set_modem_from_afc(hd_tones* t, uint32_t stream, double baud);
/* Takes, for every stream with a modem, the tuned decimated IQ of the call delivered last (what hd_stream_decimated returns), read where the call left
 * it, behind a drain of the pipeline (not from inside a callback).  A call that was pushed already adds nothing and leaves the rows as they are: HD_OK. */
int  hd_tones_push_engine(hd_tones* t);
/* Rows of cf32: stream s takes n_per_stream[s] (null: n) complex samples at d_iq + 2 * s * stride floats (stride in complex samples), from device
 * memory on the engine's GPU (8-byte aligned) or from host memory.  The buffer is the caller's again on return. */
int  hd_tones_push_device(hd_tones* t, const float* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n);
int  hd_tones_push_host(hd_tones* t, const float* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n);
/* The device rows of the last push: row s is n_per_stream[s] floats at *d_rows + s * *stride (n_per_stream: S entries, written by the call).  They are
 * valid until the next push or reset; what hd_clocked_push_device and hd_baud_probe_push_device take. */
int  hd_tones_rows(hd_tones* t, const float** d_rows, size_t* stride, uint32_t* n_per_stream);
/* A host copy of one row of the last push: returns its length and writes min(length, cap) floats.  Negative: HD_ERR_*. */
int  hd_tones_output(hd_tones* t, uint32_t stream, float* out, size_t cap);
int  hd_tones_stats(hd_tones* t, uint32_t stream, hd_tones_info* out);

/* ---- tone search: the two FSK tones of a stream that was never strong, from a long-averaged spectrum (not in the reference) ----
 * survey -> front tune -> probe -> trial -> TONE SEARCH -> tones -> hd_clocked_push_device.  The tone filters need both tones to a few per cent of the baud
 * rate; the engine's only per-stream spectrum is one 4096-sample snapshot per spectrum call, and its peaks are what the AFC misjudges on a weak signal.
 * What finds them is long integration: a Welch-averaged power spectrum per stream at the decimated rate, kept over many calls, and a two-tone detector
 * on top of it (habdec_amd_host.h: hd_host_tone_search_detect).  A tone search is attached to an engine like a tones object (its device, mutex and first
 * queue; destroy it before the engine) and reads what that one reads: each stream's tuned decimated IQ in cf32 (hd_stream_decimated).  Per stream it
 * keeps 4096 double accumulators (fftshifted), a segment count, the absolute sample index and a carry of the samples that do not yet fill a segment.
 * fsd = hd_engine_decimated_rate(e).
 *  - i = the stream's absolute sample index since its last reset, uint64.  Segment j is samples [2048 j, 2048 j + 4096) of the STREAM, not of a push:
 *    segments straddle pushes (the engine's calls leave 1024 to 4000 decimated samples each; the survey's rule, segments that never straddle pushes,
 *    would lose every one of them).  How a stream is cut into pushes does not matter, byte for byte.
 *  - Per completed segment, the survey's arithmetic: the periodic Hann float table of hd_host_survey_window, one rounded multiply per part; the engine's
 *    4096-point in-wave transform; re^2 + im^2 per bin in float, every product and sum rounded separately; the half swap, so that bin k belongs to
 *    (k - 2048) fsd / 4096.  Then acc[k] += (double)p[k], in segment order.  No float sums across segments and no floating-point atomics: this is what
 *    makes the result independent of the cut.
 *  - A NaN or Inf sample makes its segments' bins non-finite, and the accumulator stays non-finite until the stream is reset; hd_tone_search_detect
 *    reports valid = 0 for such a stream.  Other streams are untouched.
 *  - Queue, errors: as the tones object's.  One launch serves all streams, one wave per stream; a row longer than HD_TONE_SEARCH_CHUNK samples is cut into
 *    several launches in order, which changes nothing.  Every push returns when its kernels are done.  A push of more than max_push samples for a stream
 *    is HD_ERR_CAPACITY and adds nothing to any stream. */
#define HD_TONE_SEARCH_BINS 4096
#define HD_TONE_SEARCH_HOP 2048
#define HD_TONE_SEARCH_CHUNK 65536   /* samples per stream and launch: at most 32 segments per wave */
typedef struct hd_tone_search hd_tone_search;
typedef struct hd_tone_search_params {
    uint32_t max_push;         /* most samples per stream and push; default (0): the engine's largest decimated chunk per call, at least 4096 */
    uint32_t _pad;
} hd_tone_search_params;
typedef struct hd_tone_search_info {
    uint64_t samples;          /* i: samples pushed since the last reset */
    uint64_t segments;         /* segments completed since the last reset */
    uint32_t carry;            /* samples kept for the next segment: samples - 2048 segments, at most 4095 */
    uint32_t _pad;
} hd_tone_search_info;
typedef struct hd_tone_search_detect_params {
    double baud;               /* the stream's baud rate; required, > 0 */
    double shift_lo_hz;        /* least tone spacing searched; default 170 */
    double shift_hi_hz;        /* greatest tone spacing searched; default 1000 */
    double min_quality;        /* least quality for valid = 1; default 0.5 */
} hd_tone_search_detect_params;
typedef struct hd_tone_search_result {
    double   f_hi_hz, f_lo_hz; /* the upper and the lower tone at the decimated rate: what hd_tones_set_modem takes */
    double   quality;          /* the weaker tone's power above the floor over the floor's power in as many bins */
    double   floor;            /* the spectrum's median */
    uint64_t segments;
    uint32_t bin_lo;           /* the coarse search's lower bin */
    uint32_t shift_bins;       /* ... and its spacing in bins */
    uint32_t w;                /* bins per tone window, odd */
    uint32_t valid;            /* 1: both tones stand clear of the noise (habdec_amd_host.h has the rule) */
} hd_tone_search_result;
void hd_tone_search_params_default(hd_tone_search_params* p);
void hd_tone_search_detect_params_default(hd_tone_search_detect_params* p);            /* baud = 0: to be filled in */
int  hd_tone_search_create(hd_engine* e, const hd_tone_search_params* p /* null: the defaults */, hd_tone_search** out);
void hd_tone_search_destroy(hd_tone_search* ts);
int  hd_tone_search_reset(hd_tone_search* ts, uint32_t stream /* UINT32_MAX: all */);   /* accumulator, segments, sample index and carry = 0 */
/* Takes every stream's tuned decimated IQ of the call delivered last, read where the call left it, behind a drain of the pipeline (not from inside a
 * callback).  A call that was pushed already adds nothing: HD_OK.  The rules of hd_tones_push_engine. */
int  hd_tone_search_push_engine(hd_tone_search* ts);
/* Rows of cf32 as for hd_tones_push_*: stream s takes n_per_stream[s] (null: n) complex samples at d_iq + 2 * s * stride floats, from device memory on the
 * engine's GPU (8-byte aligned) or from host memory.  The buffer is the caller's again on return. */
int  hd_tone_search_push_device(hd_tone_search* ts, const float* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n);
int  hd_tone_search_push_host(hd_tone_search* ts, const float* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n);
/* p[k] = acc[k] / (segments * sum w^2), as hd_survey_power; zeros with no segment.  *segments (may be null) is always written; returns 4096, or 0 and
 * writes no power when cap < 4096.  Negative: HD_ERR_*. */
int  hd_tone_search_power(hd_tone_search* ts, uint32_t stream, double* p, size_t cap, uint64_t* segments);
int  hd_tone_search_stats(hd_tone_search* ts, uint32_t stream, hd_tone_search_info* out);
/* hd_tone_search_power followed by hd_host_tone_search_detect (habdec_amd_host.h has the algorithm and its errors). */
int  hd_tone_search_detect(hd_tone_search* ts, uint32_t stream, const hd_tone_search_detect_params* p, hd_tone_search_result* out);

/* ---- diversity combiner: several receivers of one payload, aligned and summed into one row for the clocked decoder (not in the reference) ----
 * tones -> COMBINE -> hd_clocked_push_device.  Several engine streams may be receivers of the same payload; decoded alone each fails where their sum
 * still decodes (NOTES.md has the ladder).  A combiner is attached to an engine like a tones object (its device, mutex and first queue; destroy it before
 * the engine).  Its input is one float row per engine stream -- any row hd_clocked_push_device takes: above all what hd_tones_rows hands out, but also the
 * discriminator's row -- and its output is float rows in device memory that hd_clocked_push_device takes unchanged.  Integer arithmetic behind the
 * quantisation: kernel, host restatement (hd_host_combine_*) and a numpy model agree byte for byte.
 *  - Groups: a group is 1 to HD_COMBINE_MAX_MEMBERS (8) distinct engine streams; the first is the reference r and the group is known by r.
 *    hd_combine_set_group defines a group and resets its members: every sample count 0, every delay 0, every weight 256.  A stream that was in another
 *    group leaves it; a group that loses its reference is dissolved.  count = 0 with streams[0] naming a reference dissolves that group.  A stream in no
 *    group is passed by: its samples are not counted and its row has length 0.
 *  - Per member m: a delay d_m in 0 .. HD_COMBINE_MAX_DELAY (8192) and a weight w_m in 0 .. 256.  Neither setter resets anything: the new values hold from
 *    the next push on.
 *  - Quantisation, the clocked decoder's: q = 0 for NaN, else (int32)(clamp(v, -4, 4) * 1024) truncated toward zero.  q_m(i) is member m's sample at the
 *    absolute index i since the group's last reset, 0 for i < 0.  Each member keeps its newest HD_COMBINE_RING (32768) samples on the GPU as int16.
 *  - Push: all members of a group must bring the same number of samples n in one push, else the call is HD_ERR_INVALID before anything is launched or
 *    counted (in any group).  A row above max_push: HD_ERR_CAPACITY, likewise.  One launch per HD_COMBINE_CHUNK (4096) samples of the longest row.
 *  - Output, for the group's indices j of the push: sum(j) = the sum over m of w_m q_m(j - d_m) (|sum| <= 2^23); Wt = the sum of the w_m;
 *    o = sum / max(1, Wt), truncated toward zero; the float written is o / 1024.0f, exact, and the clocked decoder's quantisation gives o back.  Row r has
 *    length n, the rows of the other members length 0.
 *  - Lag search (hd_combine_lags), over the rings -- delays and weights play no part: window N (a multiple of 64 in 1024 .. 16384), max_lag L (a multiple
 *    of 64 in 64 .. 4096), guard >= 1 in samples (the caller's bit length).  HD_ERR_UNSUPPORTED until the group has n >= N + 2 L samples.
 *    b_m(i) = 1 iff q_m(i) > 0.  For every member m != r and every l in -L .. L: A_m(l) = #{ i in [n-L-N, n-L) : b_r(i) == b_m(i + l) }, the score
 *    c_m(l) = 2 A_m(l) - N.  lag = the l of the largest score, ties to the smaller |l|, then to the negative l; peak = that score; second = the largest
 *    score over |l - lag| > guard (-N where no l is that far away); valid iff 256 peak >= min_peak_q8 N and 256 (peak - second) >= min_margin_q8 N.
 *    Meaning: the reference's sample i is the member's sample i + lag.  The reference's own entry is {lag 0, peak N, second 0, valid 1}.  RTTY's start
 *    and stop bits repeat every character, so `second` sits at a character period and is large; an unmodulated carrier scores N at every lag and has
 *    margin 0.  NOTES.md has where the defaults come from.
 *  - Align (hd_combine_align): the search, then with top = the largest lag among the valid members and 0, every valid member (the reference too) gets
 *    d_m = top - lag_m (at most 2 L <= 8192); every invalid member gets weight 0 and keeps its delay.  THE OUTPUT'S TIME AXIS MOVES WHEN DELAYS CHANGE:
 *    reset the clocked decoder behind the combiner (hd_clocked_reset of the reference's stream) after an align that changed a delay.
 *  - Queue, errors: as the tones object's; every push returns when its kernels are done. */
#define HD_COMBINE_MAX_MEMBERS 8
#define HD_COMBINE_MAX_DELAY 8192
#define HD_COMBINE_RING 32768      /* per-stream sample history on the GPU, int16 */
#define HD_COMBINE_CHUNK 4096      /* samples per stream and launch */
#define HD_COMBINE_MIN_WINDOW 1024
#define HD_COMBINE_MAX_WINDOW 16384
#define HD_COMBINE_MAX_LAG 4096
#define HD_COMBINE_NO_GROUP 0xFFFFFFFFu
typedef struct hd_combine hd_combine;
typedef struct hd_combine_params {
    uint32_t max_push;         /* samples per stream and push the rows hold; default (0): the engine's largest decimated chunk per call, at least 4096 */
    uint32_t _pad;
} hd_combine_params;
typedef struct hd_combine_lag_params {
    uint32_t window;           /* N; default 8192 */
    uint32_t max_lag;          /* L; default 2048 */
    uint32_t guard;            /* samples; required, >= 1: the bit length */
    uint32_t min_peak_q8;      /* default 76: peak / N >= 0.297, three times what noise alone reaches */
    uint32_t min_margin_q8;    /* default 16: (peak - second) / N >= 0.0625, a third of the weakest signal's margin */
} hd_combine_lag_params;
typedef struct hd_combine_lag {
    uint32_t stream;
    int32_t  lag, peak, second;
    uint32_t valid;
} hd_combine_lag;
typedef struct hd_combine_info {
    uint64_t samples;          /* n of the stream's group since its last reset; 0 in no group */
    uint32_t group;            /* the group's reference, HD_COMBINE_NO_GROUP in no group */
    uint32_t delay, weight;
    uint32_t members;          /* of the stream's group */
} hd_combine_info;
void hd_combine_params_default(hd_combine_params* p);
void hd_combine_lag_params_default(hd_combine_lag_params* p);               /* guard = 0: to be filled in */
int  hd_combine_create(hd_engine* e, const hd_combine_params* p /* null: the defaults */, hd_combine** out);   /* no stream is in a group */
void hd_combine_destroy(hd_combine* c);
/* Counts and rings of a group (by its reference; a stream that is no reference: HD_ERR_INVALID) or of all (UINT32_MAX) start again; groups, delays and
 * weights stay; the rows have length 0. */
int  hd_combine_reset(hd_combine* c, uint32_t ref /* UINT32_MAX: all */);
int  hd_combine_set_group(hd_combine* c, const uint32_t* streams, uint32_t count);
int  hd_combine_set_delay(hd_combine* c, uint32_t stream, uint32_t delay);     /* HD_ERR_INVALID: above HD_COMBINE_MAX_DELAY, or a stream in no group */
int  hd_combine_set_weight(hd_combine* c, uint32_t stream, uint32_t weight);   /* HD_ERR_INVALID: above 256, or a stream in no group */
/* The discriminator rows of the call delivered last (what hd_stream_demodulated returns), with the rules of hd_clocked_push_engine: a call that was
 * pushed already adds nothing and leaves the rows as they are. */
int  hd_combine_push_engine(hd_combine* c);
/* Rows of float as for hd_clocked_push_*: stream s takes n_per_stream[s] (null: n) floats at rows + s * stride. */
int  hd_combine_push_device(hd_combine* c, const float* d_rows, size_t stride, const uint32_t* n_per_stream, uint32_t n);
int  hd_combine_push_host(hd_combine* c, const float* rows, size_t stride, const uint32_t* n_per_stream, uint32_t n);
/* The device rows of the last push, exactly as hd_tones_rows: the triple goes straight into hd_clocked_push_device. */
int  hd_combine_rows(hd_combine* c, const float** d_rows, size_t* stride, uint32_t* n_per_stream);
/* A host copy of one row of the last push: returns its length and writes min(length, cap) floats.  Negative: HD_ERR_*. */
int  hd_combine_output(hd_combine* c, uint32_t stream, float* out, size_t cap);
int  hd_combine_stats(hd_combine* c, uint32_t stream, hd_combine_info* out);
/* The lag search of the group with reference ref: writes one entry per member, the reference's first, in the group's order; HD_ERR_INVALID where cap is
 * below the group's member count.  HD_OK, or HD_ERR_*. */
int  hd_combine_lags(hd_combine* c, uint32_t ref, const hd_combine_lag_params* p, hd_combine_lag* out, size_t cap);
/* hd_combine_lags, then the align step.  Returns the number of valid entries (the reference's among them), or HD_ERR_*. */
int  hd_combine_align(hd_combine* c, uint32_t ref, const hd_combine_lag_params* p, hd_combine_lag* out, size_t cap);

/* ---- SSDV packets: Reed-Solomon decoding with soft erasures (the reference's ssdv_callback_ side channel; built from the published format) ----
 * tones -> combine -> clocked -> SSDV.  Picture payloads send the same RTTY bytes as telemetry, but as 256-byte SSDV packets, each an RS(255,223)
 * codeword behind a sync byte.  An SSDV object is attached to an engine like a clocked decoder (its device, mutex and first queue; destroy it before the
 * engine).  Its input is bytes with a confidence each -- above all the clocked decoder's records, whose soft values say which bytes to erase and whose
 * positions say where a character was lost -- and its output is whole corrected packets, the 256 bytes an SSDV server takes.  JPEG reassembly is not
 * built, and the facade's ssdv_callback_ still never fires.  No copy of the fsphil/ssdv library is at hand: agreement with it rests on the published
 * format alone.  Kernel (kernels/ssdv.hip), host restatement (hd_host_ssdv_*) and a numpy model agree byte for byte on all of the following.
 *  - Stream: per engine stream a sequence of pairs (b_i, c_i); i is the absolute byte index since the stream's last reset (uint64), b_i a byte, c_i a
 *    confidence in 0 .. 0xFFFFFF (the push doors saturate it).  How a stream is cut into pushes and scans cannot matter.
 *  - Code: GF(2^8) modulo x^8 + x^7 + x^2 + x + 1 (0x187), alpha = 0x02.  The received word of candidate i is r_j = b_{i+j}, j = 1 .. 255; as a
 *    polynomial r_1 is the coefficient of x^254 and r_255 that of x^0.  A codeword is a word whose polynomial vanishes at alpha^(11 (112 + m)),
 *    m = 0 .. 31: the CCSDS (255,223) code in the conventional basis.  Bytes 1 .. 223 are data, 224 .. 255 parity.  CRC: CRC-32 (reflected, polynomial
 *    0xEDB88320, initial value and final xor 0xFFFFFFFF) over bytes 1 .. 219, stored big-endian in bytes 220 .. 223.  Byte 0 is the sync byte 0x55; no
 *    code covers it.  (The generator polynomial is palindromic, 1, 91, 127, 86, 16, 30, ...; an encoded packet has 32 zero syndromes.)
 *  - Candidates: position i is decided once i + 256 <= n, n = bytes pushed.  Every position is a candidate: a sync gate would throw away packets the
 *    code can repair.
 *  - Trials, in this order, the first that succeeds wins.  No-FEC: if b_i == 0x55 and b_{i+1} == 0x67 and the CRC of bytes 1 .. 219 as received
 *    matches: trial = HD_SSDV_NOFEC (255), nothing corrected.  Then t = 0, 1, 2, 3 with f_t = 0, 8, 16, 24 erasures: E_t is the set of the f_t positions
 *    j in 1 .. 255 with the smallest key (c_{i+j} << 8) | j.  The trial succeeds iff there is a codeword w with e = |{ j not in E_t : w_j != r_j }| and
 *    2 e + f_t <= 32 (such a w is unique) and w's CRC matches.  A codeword whose CRC is wrong: crc_bad += 1 and the next trial runs.  (A decoder may
 *    skip work whose outcome it knows -- 32 zero syndromes, say; the outcomes are what is defined.)
 *  - Packet: pos = i, trial, errors = e, erasures = f_t, erasures_changed = the erased positions whose byte changed, type = w_1, data[256] = 0x55
 *    followed by w (even where b_i was something else), and the header: callsign from bytes 2 .. 5, a big-endian uint32 in base 40, digits taken least
 *    significant first while the value is not 0 (0 '-', 1 .. 10 '0' .. '9', 11 .. 13 '-', 14 .. 39 'A' .. 'Z'); image id byte 6; packet id bytes 7 .. 8
 *    big-endian; width byte 9 * 16; height byte 10 * 16; flags byte 11; MCU offset byte 12; MCU index bytes 13 .. 14 big-endian.  After the CRC no field
 *    is tested for plausibility.
 *  - Delivery: per stream, results are taken in increasing pos; a result with pos < (pos of the last delivered packet) + 256 is dropped, overlaps += 1.
 *    Which packets a scan delivers does not depend on the order in which waves finish.  Packets wait on the host until hd_ssdv_take_packets.
 *  - Counters per stream: bytes (n, fillers among them), decided, fillers, crc_bad, overlaps, packets[5] (delivered, by trial 0 .. 3, then no-FEC).
 *  - False accepts: a random word decodes to some codeword with probability 2.6e-14, 9.9e-10, 1.2e-5 and 2.6e-2 at f = 0, 8, 16, 24 (NOTES.md derives
 *    it: below 1e-4 up to f = 16, not at 24), and the CRC-32 then passes with probability 2^-32: 6e-12 per candidate over the four trials, beside the
 *    clocked decoder's 0.14 % per failed match.
 *  - Doors: the push doors append on the host; a scan uploads what is new, launches once for all streams (in chunks of at most HD_SSDV_LAUNCH
 *    candidates), waits and collects.  hd_ssdv_push_records: b = ch & 0xFF, c = min(0xFFFFFF, min over k < 8 of |data_k|).  Gap rule: the door remembers
 *    the pos of the stream's last record across pushes; for a record at pos after one at prev, k = (pos - prev + char_len / 2) / char_len in integer
 *    division; if 2 <= k <= 1 + max_fill, k - 1 fillers (b = 0, c = 0) go in front of the record and fillers += k - 1; a larger k is a pause in
 *    transmission and inserts nothing; char_len = 0 switches the rule off.  hd_ssdv_push_clocked: for every stream whose clocked modem has 8 data bits
 *    it takes all waiting records exactly as hd_clocked_records does (they pass through the clocked text stage, so sentences are unaffected), pushes
 *    them with char_len = (K F + 32768) >> 16 of that stream's clock, then scans; streams with 7 data bits are passed by.
 *  - Queue, errors: as the clocked decoder's; a scan returns when its kernels are done. */
#define HD_SSDV_NOFEC 255u         /* hd_ssdv_packet.trial of a packet accepted without the code */
#define HD_SSDV_TYPE_NOFEC 0x67u
#define HD_SSDV_RING 4096          /* per-stream bytes on the GPU */
#define HD_SSDV_LAUNCH 16384       /* candidates per launch over all streams */
typedef struct hd_ssdv hd_ssdv;
typedef struct hd_ssdv_params {
    uint32_t max_fill;         /* the gap rule's longest run of fillers; default 7, at most 64, 0: none */
    uint32_t _pad;
} hd_ssdv_params;
typedef struct hd_ssdv_packet {
    uint64_t pos;
    uint32_t trial;            /* 0 .. 3, or HD_SSDV_NOFEC */
    uint32_t errors, erasures, erasures_changed;
    uint32_t type;
    uint32_t image_id, packet_id, width, height, flags, mcu_offset, mcu_index;
    char     callsign[8];      /* NUL-terminated */
    uint8_t  data[256];
} hd_ssdv_packet;
typedef struct hd_ssdv_counters {
    uint64_t bytes, decided, fillers, crc_bad, overlaps;
    uint64_t packets[5];
} hd_ssdv_counters;
void hd_ssdv_params_default(hd_ssdv_params* p);
int  hd_ssdv_create(hd_engine* e, const hd_ssdv_params* p /* null: the defaults */, hd_ssdv** out);   /* HD_ERR_UNSUPPORTED: more than HD_SSDV_LAUNCH streams */
void hd_ssdv_destroy(hd_ssdv* v);
/* Bytes, counters, the gap rule's memory and the delivery's last pos of the stream start again; packets not yet taken stay. */
int  hd_ssdv_reset(hd_ssdv* v, uint32_t stream /* UINT32_MAX: all */);
int  hd_ssdv_push_bytes(hd_ssdv* v, uint32_t stream, const uint8_t* bytes, const uint32_t* conf /* null: every c = 0xFFFFFF */, size_t n);
int  hd_ssdv_push_records(hd_ssdv* v, uint32_t stream, const hd_clocked_record* records, size_t n, uint32_t char_len);
/* HD_ERR_INVALID unless both objects belong to one engine. */
int  hd_ssdv_push_clocked(hd_ssdv* v, hd_clocked* c);
int  hd_ssdv_scan(hd_ssdv* v);
/* Hands out up to cap of the stream's waiting packets, oldest first, and returns how many were written; out null: how many wait.  Negative: HD_ERR_*. */
int  hd_ssdv_take_packets(hd_ssdv* v, uint32_t stream, hd_ssdv_packet* out, size_t cap);
int  hd_ssdv_stats(hd_ssdv* v, uint32_t stream, hd_ssdv_counters* out);

/* ---- Horus Binary 4FSK: tone bank, frame search on a timing grid, soft Golay(23,12) (not in the reference; built from the published format) ----
 * survey -> front tune -> FSK4.  A second modulation beside RTTY: 4FSK at about 100 baud, a 22- or 32-byte payload, Golay(23,12) parity, interleaved and
 * scrambled behind the unique word 0x24 0x24.  An fsk4 object is attached to an engine like a tones object (its device, mutex and first queue; destroy
 * it before the engine) and reads the same input, each stream's tuned decimated cf32 IQ, through the same three doors.  Frames leave through
 * hd_fsk4_take_frames alone, never through the sentence callbacks.  horusdemodlib is not at hand: agreement with it rests on the format as restated
 * here alone, and every format constant is a field of hd_fsk4_frame.  Kernels (kernels/fsk4.hip), host restatement (hd_host_fsk4_*) and a numpy model
 * (tests/fsk4_model.py) agree byte for byte on all of the following.  fsd = hd_engine_decimated_rate(e).
 *  - On air: bytes go most significant bit first, two bits make a symbol, first bit high; symbol value v is the tone f0 + v spacing (natural binary).
 *  - Frame: the unique word uw[0] uw[1], then a body of B = P + ceil(11 K / 8) bytes, P = payload_bytes, K = ceil(8 P / 12): 4 (2 + B) symbols.
 *    HD_FSK4_HORUS_V1: P 22, K 15, B 43, 180 symbols; HD_FSK4_HORUS_V2: P 32, K 22, B 63, 260 symbols.
 *  - Body before interleaving: the payload, then the parity bit stream.  Codeword k has the 12 data bits 12 k .. 12 k + 11 of the payload, bytes taken
 *    most significant bit first, zeros past the payload's end; its 11 parity bits are the remainder of data x^11 by golay_poly (0xC75), appended most
 *    significant first to the parity stream, whose last byte is zero-padded.  As a 23-bit word a codeword is data << 11 | parity.
 *  - Interleaver: body bits are numbered i <-> byte i / 8, bit i % 8 (least significant first, unlike the on-air order); bit i moves to
 *    j = interleave_mul i mod 8 B (337 and 503: the largest primes below 344 and 504).
 *  - Scrambler, after the interleaver, same numbering: a 15-bit state, scrambler_seed (0x4A80) at every frame start; out = bit 1 ^ bit 0, then
 *    state = state >> 1 | out << 14; body bit i is xored with the i-th output (0,0,0,0,0,0,1,1,1,1,1,1,0,1,1,0, ...).
 *  - Payload check: the last two payload bytes are CRC16-CCITT (0x1021, initial value 0xFFFF, nothing reflected, no final xor) over the first P - 2,
 *    low byte first.
 *  - Modem (hd_fsk4_set_modem): F = floor(fsd / baud * 65536 + 0.5); HD_ERR_UNSUPPORTED unless 8 <= fsd / baud <= HD_FSK4_MAX_SPB and the frame is one the
 *    decoder can take (3 <= P <= 32, interleave_mul coprime with 8 B, a nonzero 15-bit seed, golay_poly a divisor of x^23 + 1 of degree 11);
 *    Phi_t = (uint32)(int64)nearbyint((f0 + t spacing) / fsd * 2^32), t = 0 .. 3, HD_ERR_INVALID unless every tone lies inside +-fsd / 2;
 *    W = max(1, (F window_q8 + 2^23) >> 24): the whole symbol by default, because the timing is recovered.  Psi_t = 0.  The tones
 *    come from the caller or from the tracker below (hd_fsk4_track_*).
 *  - Retune (hd_fsk4_retune): new Phi_t by the modem's rule (HD_ERR_INVALID: a tone outside +-fsd / 2, a stream without a modem) come into force at
 *    sample at_sample with Psi_t += at_sample (Phi_old - Phi_new) mod 2^32, so every rotator's phase is continuous and a small step costs no symbol.
 *    Baud, frame, slots, rings, counters and the open group stay.  Retunes wait per stream on the host and take effect in the order of the calls; a
 *    push is cut at at_sample and the state is updated on the queue between the two launches.  An at_sample behind the stream's index takes effect
 *    at once, at that index, and counts as late (hd_fsk4_retune_stats).  A reset drops the waiting retunes and keeps the tones in force.
 *  - Per sample i (uint64 since the stream's last reset): the tones object's rules for four tones -- q = 0 for NaN, else (int32)(clamp(v, -8, 8) * 256);
 *    a = (uint32)(i Phi_t + Psi_t) >> 22; r_re = (q_re C[a] + q_im C[(a + 768) & 1023]) >> 15, r_im = (q_im C[a] - q_re C[(a + 768) & 1023]) >> 15 with the
 *    probe's table C; running sums mod 2^32; A_t(i) = floor(sqrt(re^2 + im^2)) of the sums over the W samples up to i (fewer in front of sample 0).
 *  - Slots: a timing grid of eight phases per symbol, slot g = 8 k + p.  Slot g's record is (A_0, A_1, A_2, A_3) at its last sample
 *    end(g) = ((g + 8) F >> 19) - 1, four uint32; it exists once that sample is pushed.  Records go to a per-stream ring on the GPU.
 *  - Candidates: every slot g is one, a frame whose symbol m is slot g + 8 m.  It is decided by the first scan after its last slot exists, exactly
 *    once; every push ends with a scan, and what comes out does not depend on how the samples were cut into pushes.
 *      1. Hard symbol: argmax_t A_t, the lowest t on ties.
 *      2. Unique-word gate: the 16 hard bits of the first 8 symbols differ from the unique word in at most uw_max_errors bits, or the candidate ends here.
 *      3. Soft bits of symbol m: hi = max(A_2, A_3) - max(A_0, A_1), lo = max(A_1, A_3) - max(A_0, A_2); a hard bit is soft > 0, its confidence |soft|.
 *      4. On-air bit r of the body is body byte r / 8, bit 7 - r % 8; descrambling negates, de-interleaving permutes; K words of 23 soft values are
 *         gathered; the zero-padded data positions of the last word are hard 0 with confidence 2^24.
 *      5. Soft Golay, per word: the chase_bits least confident positions (ties: the one nearer the most significant bit first) are position 0, 1, ...
 *         of a flip pattern; for each of the 2^chase_bits patterns, lowest number first, the hard word with the pattern's positions flipped is decoded to
 *         the one codeword within distance 3 (syndrome table, made at set_modem); its cost is the sum of the confidences where it differs from the
 *         unflipped hard word.  The lowest cost wins, the earlier pattern on ties.  corrected = the bits in which the winners differ from the hard words.
 *      6. crc_ok: the CRC16 of the decoded payload matches.  metric = the sum over the frame's symbols of max_t A_t.
 *  - Guard against noise: the code is perfect, so step 5 never fails, and gate and CRC alone pass about 3e-8 of noise candidates.
 *    A frame is refused when corrected > max_corrected (default 2 K: noise corrects about 2.85 bits per word, a frame at 5 % bit errors about 1.2).
 *  - Selection: only candidates with crc_ok within max_corrected count.  The first of them opens a group; those less than 16 slots (two symbols: the
 *    neighbouring timing phases of one frame) behind it contest the delivery -- fewest corrected bits, then the largest metric, then the lowest slot
 *    -- and the best is delivered once every slot of that contest is decided, two symbols behind the frame's end.  A later candidate less than
 *    8 (symbols - 1) slots behind the delivered one overlaps that frame (the next frame may follow at once, and its early phases with it) and is
 *    dropped, overlaps += 1; the next one opens the next group.  (A contest as long as the frame would hold every frame back by its own length.)
 *    Frames wait on the host, per stream in increasing position, until hd_fsk4_take_frames.
 *  - Counters per stream: samples, slots, candidates (decided), gate_passes, crc_failures, refused (by max_corrected), overlaps, frames.
 *  - Queue, errors: as the tones object's; a push returns when its kernels are done.  A push longer than max_push: HD_ERR_CAPACITY.  A row longer than
 *    HD_FSK4_CHUNK samples is cut into launches; a scan's candidates into launches of at most HD_FSK4_LAUNCH over all streams.
 *  - Not built: timing finer than a slot, the payload's fields and upload bodies, 2FSK Horus, feeding the combiner. */
#define HD_FSK4_MAX_SPB 2048
#define HD_FSK4_CHUNK 4096         /* samples of a row per launch of the slot kernel */
#define HD_FSK4_LAUNCH 16384       /* candidates per launch of the frame kernel over all streams */
#define HD_FSK4_MAX_PAYLOAD 32
#define HD_FSK4_HORUS_V1 1
#define HD_FSK4_HORUS_V2 2
typedef struct hd_fsk4 hd_fsk4;
typedef struct hd_fsk4_frame {
    uint32_t payload_bytes;    /* P */
    uint8_t  uw[2];
    uint16_t _pad;
    uint32_t interleave_mul, scrambler_seed, golay_poly;
} hd_fsk4_frame;
typedef struct hd_fsk4_params {
    uint32_t max_push;         /* longest push per stream in samples; 0: what the engine's longest call leaves, or 4096; at most 2^22 */
    uint32_t window_q8;        /* the tone filters' window in 1/256 symbols, 32 .. 256; default 256 */
    uint32_t uw_max_errors;    /* 0 .. 4; default 2 */
    uint32_t chase_bits;       /* 0 .. 6; default 4 */
    int32_t  max_corrected;    /* a frame with more corrected bits is refused; negative (the default): 2 K of the stream's frame */
    uint32_t _pad;
} hd_fsk4_params;
typedef struct hd_fsk4_rx {    /* one delivered frame */
    uint64_t slot;             /* the frame's first slot, 8 k + phase */
    uint64_t start_sample;     /* the first sample of its first symbol: slot F >> 19 */
    uint64_t metric;
    uint32_t payload_bytes, corrected, phase, uw_errors;
    uint8_t  payload[HD_FSK4_MAX_PAYLOAD];
} hd_fsk4_rx;
typedef struct hd_fsk4_candidate {   /* one candidate behind the unique-word gate, whatever became of it (the restatement's and the test hooks' record) */
    uint64_t slot, metric;
    uint32_t crc_ok, corrected, uw_errors, _pad;
    uint8_t  payload[HD_FSK4_MAX_PAYLOAD];
} hd_fsk4_candidate;
typedef struct hd_fsk4_counters {
    uint64_t samples, slots, candidates, gate_passes, crc_failures, refused, overlaps, frames;
    uint32_t F, W, step[4];    /* the modem's integers: F = 0, no modem */
    uint32_t symbols, codewords;
} hd_fsk4_counters;
void hd_fsk4_params_default(hd_fsk4_params* p);
/* The two presets.  HD_ERR_UNSUPPORTED: no such preset. */
int  hd_fsk4_frame_preset(int preset, hd_fsk4_frame* out);
int  hd_fsk4_create(hd_engine* e, const hd_fsk4_params* p /* null: the defaults */, hd_fsk4** out);   /* HD_ERR_UNSUPPORTED: window_q8, more than HD_FSK4_LAUNCH streams */
void hd_fsk4_destroy(hd_fsk4* f);
/* Samples, slots, candidates, counters and the open group of the stream start again; the modem stays, and so do frames not yet taken. */
int  hd_fsk4_reset(hd_fsk4* f, uint32_t stream /* UINT32_MAX: all */);
int  hd_fsk4_set_modem(hd_fsk4* f, uint32_t stream, double baud, double f0_hz, double spacing_hz, const hd_fsk4_frame* frame);   /* resets the stream */
/* The three doors of the tones object, with its rules; each ends with a scan. */
int  hd_fsk4_push_engine(hd_fsk4* f);
int  hd_fsk4_push_device(hd_fsk4* f, const float* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n);
int  hd_fsk4_push_host(hd_fsk4* f, const float* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n);
/* Decides every candidate whose last slot exists and is not decided yet.  Every push ends with one, so on its own it finds nothing left: HD_OK. */
int  hd_fsk4_scan(hd_fsk4* f);
/* Hands out up to cap of the stream's waiting frames, oldest first, and returns how many were written; out null: how many wait.  Negative: HD_ERR_*. */
int  hd_fsk4_take_frames(hd_fsk4* f, uint32_t stream, hd_fsk4_rx* out, size_t cap);
int  hd_fsk4_stats(hd_fsk4* f, uint32_t stream, hd_fsk4_counters* out);
typedef struct hd_fsk4_retune_info {
    uint64_t retunes, late, waiting;   /* retunes that took effect since the stream's last reset; those of them that were late; those that wait */
    uint32_t psi[4];                   /* the phase words in force */
} hd_fsk4_retune_info;
/* Moves the stream's four tones at at_sample without a reset (see "Retune" above). */
int  hd_fsk4_retune(hd_fsk4* f, uint32_t stream, double f0_hz, double spacing_hz, uint64_t at_sample);
int  hd_fsk4_retune_stats(hd_fsk4* f, uint32_t stream, hd_fsk4_retune_info* out);

/* ---------------------------------------------------------------------------------------------------------------------------------------------------
 * 4FSK tone tracker.  A payload's oscillator is a few hundred Hz off when it starts and moves by more than the modem's tolerance (0.1 baud for nothing
 * lost, NOTES.md) during a flight.  A tracker keeps, per stream, a Welch-averaged spectrum of the decimated IQ -- the tone search's kernel and segments,
 * accumulators of its own -- and at the end of every epoch looks for four equally spaced tones in it (kernels/fsk4_track.hip: k_fsk4_comb, one
 * workgroup per stream, one launch for every stream whose epoch ended); attached to an fsk4 object it retunes that object's streams.  Attached to an
 * engine like a tones object; destroy it before the engine.  Kernel, host restatement (hd_host_fsk4_comb_detect, hd_host_fsk4_track_*) and a numpy
 * model (tests/fsk4_track_model.py) agree byte for byte on the detector, which is integer arithmetic behind the quantisation.  bin = fsd / 4096; bin
 * index k belongs to f = (k - 2048) bin.  In this order:
 *   1. Non-finite input: any non-finite sum, or a maximum that is not > 0, gives valid = 0 and every other field 0.
 *   2. Quantisation: q[k] = (uint32)floor(acc[k] / max(acc) * 2^19), one double division per bin (0 for a negative sum); prefix sums fit 32 bits.
 *   3. Floor: the lower median of q (element 2047 of the sorted bins).
 *   4. Window: w = max(3, (int)nearbyint(0.5 baud / bin) | 1) bins, the two-tone detector's; h = w / 2.
 *   5. Coarse search: spacing d in quarter bins, d_lo = ceil(4 spacing_lo / bin) .. d_hi = floor(4 spacing_hi / bin); the lowest centre c0 in whole
 *      bins; centre t is c0 + ((t d + 2) >> 2), and all four windows lie inside the band b_lo = 2048 + ceil(f_lo / bin) .. b_hi = 2048 + floor(f_hi /
 *      bin) (clipped to 0 .. 4095): c0 - h >= b_lo, centre 3 + h <= b_hi.  A candidate's score is the weakest of its four window sums of q -- a lone
 *      carrier, an RTTY pair or three tones of four score like noise.  The largest score wins, then the lowest d, then the lowest c0.
 *   6. Refinement, per tone, four rounds from c = the coarse centre: over the bins m within +-w of c (inside 0 .. 4095) with weights
 *      max(q[m] - floor, 0), sw = sum of the weights, sm = sum of (m - c) weight; centroid = 256 c + floor((512 sm + sw) / (2 sw)) in 1/256 bin (256 c
 *      where sw = 0); the next round's c = (centroid + 128) >> 8.
 *   7. Fit: the least-squares line through the four centroids c_t: S10 = -3 c_0 - c_1 + c_2 + 3 c_3, spacing_q8 = floor((S10 + 5) / 10),
 *      f0_q8 = floor((5 (c_0 + c_1 + c_2 + c_3) - 3 S10 + 10) / 20).
 *   8. Known spacing (spacing_lo == spacing_hi): d = nearbyint(4 spacing / bin) alone is searched, spacing_q8 = 64 d and only f0 is fitted,
 *      f0_q8 = floor((c_0 + c_1 + c_2 + c_3 - 6 spacing_q8 + 2) / 4).
 *   9. Quality: quality_q8 = floor(256 (score - w floor) / max(w floor, 1)), 0 where the score is below w floor.  valid = quality_q8 >= min_quality_q8
 *      and the stream has at least min_segments effective segments.
 *  In Hz: f0_hz = (f0_q8 / 256 - 2048) bin, spacing_hz = spacing_q8 / 256 bin, tone t = f0_hz + t spacing_hz.
 *  A spacing below 2 baud is HD_ERR_UNSUPPORTED (the tones' lobes overlap and the spectrum is nearly flat over four baud); a band or a spacing range
 *  that leaves no candidate is HD_ERR_INVALID.
 *  Epochs: an epoch of a stream is epoch_segments consecutive segments by the stream's absolute segment index (segment j is samples 2048 j ..
 *  2048 j + 4095), so epoch e ends with sample 2048 ((e + 1) epoch_segments + 1), its end sample.  A push is cut into rounds so that no spectrum launch
 *  crosses a stream's epoch end; after a round k_fsk4_comb runs for the streams whose epoch ended in it and then multiplies their accumulators by
 *  decay_q8 / 256 (one rounding per bin).  The effective segment count goes the same way on the host: + epoch_segments, the test, * decay_q8 / 256.
 *  Records, estimates and accumulators do not depend on how the samples were cut into pushes.  A stream without hd_fsk4_track_set_stream takes no samples.
 *  Closing the loop (hd_fsk4_track_attach): after every epoch with a valid record one of whose tones differs from the attached modem's by more than
 *  deadband / 256 baud, the tracker calls hd_fsk4_retune with at_sample = the epoch's end sample.  Both objects count samples from the same reset; per
 *  call, push the tracker first, then the fsk4 object: in that order no retune is late and the decode does not depend on the cut.  A stream without a
 *  modem is left alone; acquisition from nominal tones is a retune like any other.
 *  Not built: narrowing the search around a lock, spacings below 2 baud, 2FSK. */
typedef struct hd_fsk4_track hd_fsk4_track;
typedef struct hd_fsk4_track_params {
    uint32_t max_push;         /* as the tone search's */
    uint32_t epoch_segments;   /* default 4 */
    uint32_t decay_q8;         /* 0 .. 256: what an epoch leaves of the sums for the next; default 128 */
    uint32_t min_quality_q8;   /* default 192 (NOTES.md has the measurements on either side) */
    uint32_t min_segments;     /* default 4 */
    uint32_t deadband;         /* 1/256 baud; default 8 */
} hd_fsk4_track_params;
typedef struct hd_fsk4_comb_params {   /* what hd_host_fsk4_comb_detect takes: one stream's search, and the two validity tests */
    double baud, spacing_lo_hz, spacing_hi_hz, f_lo_hz, f_hi_hz;
    uint32_t min_quality_q8, segments_ok;
} hd_fsk4_comb_params;
typedef struct hd_fsk4_comb_record {
    int32_t  f0_q8, spacing_q8;        /* 1/256 bin; f0 on the bin index */
    uint32_t c0, d, w, floor, score, quality_q8, valid;
    int32_t  centroid_q8[4];
    uint32_t _pad[3];
} hd_fsk4_comb_record;
typedef struct hd_fsk4_track_est {
    hd_fsk4_comb_record rec;
    double   f0_hz, spacing_hz;
    uint64_t end_sample, epoch;        /* the record's epoch: its end sample and its number from 0 */
} hd_fsk4_track_est;
typedef struct hd_fsk4_track_info {
    uint64_t samples, segments, epochs, valid_epochs, retunes;
} hd_fsk4_track_info;
void hd_fsk4_track_params_default(hd_fsk4_track_params* p);
int  hd_fsk4_track_create(hd_engine* e, const hd_fsk4_track_params* p /* null: the defaults */, hd_fsk4_track** out);
void hd_fsk4_track_destroy(hd_fsk4_track* tr);
int  hd_fsk4_track_reset(hd_fsk4_track* tr, uint32_t stream /* UINT32_MAX: all */);   /* sums, counts, carry and records; the stream's search stays */
/* Gives the stream its search (and resets it).  HD_ERR_UNSUPPORTED: spacing_lo_hz < 2 baud; HD_ERR_INVALID: nothing to search. */
int  hd_fsk4_track_set_stream(hd_fsk4_track* tr, uint32_t stream, double baud, double spacing_lo_hz, double spacing_hi_hz, double f_lo_hz, double f_hi_hz);
int  hd_fsk4_track_attach(hd_fsk4_track* tr, hd_fsk4* f /* null: detach */);   /* an fsk4 object of the same engine; destroy the tracker first */
/* The three doors of the tone search, with its rules. */
int  hd_fsk4_track_push_engine(hd_fsk4_track* tr);
int  hd_fsk4_track_push_device(hd_fsk4_track* tr, const float* d_iq, size_t stride, const uint32_t* n_per_stream, uint32_t n);
int  hd_fsk4_track_push_host(hd_fsk4_track* tr, const float* iq, size_t stride, const uint32_t* n_per_stream, uint32_t n);
/* The newest record; HD_ERR_UNSUPPORTED while the stream has none. */
int  hd_fsk4_track_estimate(hd_fsk4_track* tr, uint32_t stream, hd_fsk4_track_est* out);
int  hd_fsk4_track_stats(hd_fsk4_track* tr, uint32_t stream, hd_fsk4_track_info* out);

/* ---- APRS: Bell 202 AFSK carrying AX.25 UI frames -- tone pair, HDLC flag search on a timing grid, CRC-guided repair (not in the reference) ----
 * survey -> front tune -> hd_stream_set_lowpass_bw wide enough for the FM signal -> afsk.  The third modulation: the stream's polar discriminator is
 * an FM demodulator, and with the low-pass opened its row (hd_stream_demodulated) is the audio a packet modem takes.  An afsk object is attached to an
 * engine like a clocked decoder (its device, mutex and first queue; destroy it before the engine) and reads the same float rows through the same three
 * doors with the same rules.  Frames leave through hd_afsk_take_frames alone, never through the sentence callbacks.  No other TNC is at hand:
 * agreement with them rests on the published AX.25 / Bell 202 format as restated here.  Kernels (kernels/afsk.hip), host restatement (hd_host_afsk_*)
 * and a numpy model (tests/afsk_model.py) agree byte for byte on all of the following.  fsd = hd_engine_decimated_rate(e); every index is absolute per
 * stream since its last reset (uint64); how the samples are cut into pushes matters to no record, frame or counter.
 *  - On air: a frame is flag(s) 0x7E, the bytes least significant bit first with a 0 stuffed behind every five 1s, flag(s); NRZI: a 0 is a change of
 *    tone, a 1 none.  A UI frame is destination, source and up to eight digipeater addresses of seven bytes (six characters << 1, then the SSID byte
 *    0b?11ssss? whose bit 0 is set in the last address and whose bit 7 is the digipeater's H bit), control 0x03, PID 0xF0, the information, the FCS.
 *  - Modem (hd_afsk_set_modem; it resets the stream): F = floor(fsd / baud * 65536 + 0.5); W = (F + 32768) >> 16, one bit;
 *    Phi_t = (uint32)(int64)nearbyint(f_t / fsd * 2^32) for mark and space.  HD_ERR_UNSUPPORTED unless 8 <= fsd / baud <= HD_AFSK_MAX_SPB;
 *    HD_ERR_INVALID unless 0 < mark, space < fsd / 2 and mark != space.  hd_afsk_set_bell202: 1200 baud, 1200 / 2200 Hz; the 300 baud HF pair is
 *    hd_afsk_set_modem(a, s, 300, 1600, 1800).  After create no stream has a modem, and a stream without one is passed by.
 *  - Sample: q = 0 for NaN, else (int32)(clamp(v, -4, 4) * 1024) truncated toward zero, the clocked decoder's rule.
 *  - Tone pair, per tone t: a = (uint32)(i Phi_t) >> 22; r_re = (q C[a]) >> 15, r_im = (-q C[(a + 768) & 1023]) >> 15 with the probe's table C and
 *    arithmetic shifts; running sums mod 2^32 over the W samples up to i (samples in front of index 0 are zero); A_t(i) = floor(sqrt(re^2 + im^2));
 *    d(i) = A_mark(i) - A_space(i), an int32.
 *  - Slots: eight phases per bit, slot g = 8 k + p, which ends at sample end(g) = ((g + 8) F >> 19) - 1.  Its record is d(end(g)); it exists once
 *    that sample is pushed.  Records go to a per-stream ring of HD_AFSK_RING slots on the GPU.
 *  - Bits, per phase: level l_k = (d > 0); NRZI data bit n_k = (l_k == l_{k-1}); the confidence of a level is |d|.
 *  - Candidate: every slot g = 8 k + p >= 64 at which n_{k-7} .. n_k = 0,1,1,1,1,1,1,0 on hard levels -- a flag whose last bit is k.  It is decided
 *    exactly once, by the first scan after slot g + 8 L exists, L = ceil(8 max_frame_bytes 6 / 5) + 8 bits; every push ends with a scan.  The rule is
 *    fixed, so that the state after n samples is a function of those samples; a smaller max_frame_bytes buys latency.
 *  - Walk from bit k + 1 with a count of consecutive 1s: a 1 is kept, the seventh consecutive 1 ends the walk (HD_AFSK_ABORT); a 0 after exactly
 *    five 1s is dropped (stuffed); a 0 after six 1s closes the frame, and the last seven kept bits (a 0 and six 1s) belong to the flag; any other 0 is
 *    kept.  No closing flag within L bits: HD_AFSK_OPEN.  The kept bits in front of the closing flag, least significant bit first, are the frame; it
 *    is shaped iff their count is a multiple of 8 and HD_AFSK_MIN_FRAME <= bytes <= max_frame_bytes, FCS included (else HD_AFSK_UNSHAPED; two flags
 *    in a row give a zero-length frame, which is not shaped).
 *  - FCS: the last two frame bytes are CRC-16/X-25 over the rest (reflected 0x8408, initial 0xFFFF, final xor 0xFFFF, low byte first; its check
 *    value over "123456789" is 0x906E).
 *  - Address check: the address field ends at the first byte with bit 0 set; its index must be 7 m - 1 with 2 <= m <= 10 and lie in front of the
 *    FCS.  Every callsign byte (the first six of each address) has bit 0 clear and byte >> 1 in 'A'-'Z', '0'-'9' or ' '.
 *  - Repair, for a shaped frame whose FCS fails: the list is the repair_bits levels with the smallest |d| among the levels of bit k + 1 up to the bit
 *    in front of the closing flag's eight, ties to the earlier bit.  All subsets of size 1, then 2, up to repair_flips are tried in the list's
 *    lexicographic order; with the untouched pattern they number at most 64 (1 + 8 + 28 = 37 by default), or create refuses.  A pattern flips
 *    levels, so each flip changes two NRZI bits and may move stuffing: its walk is run afresh.  A pattern counts iff its walk is shaped, closes at
 *    the same bit as the hard walk, its FCS agrees and its address field passes the check.  The first pattern that counts wins
 *    (HD_AFSK_REPAIRED, flips = the subset's size).  Either limit 0: no repair.  No pattern counts: HD_AFSK_REFUSED if one of them failed at
 *    the address check alone, else HD_AFSK_FCS_FAILED.
 *  - Plain frames (HD_AFSK_PLAIN: shaped, FCS right on hard levels) must pass the address check when require_addr is set (else HD_AFSK_REFUSED);
 *    without it they are delivered with addr_ok = 0.  In noise about 2^-8 of the bit positions of a phase are flags, roughly a percent of those walk to
 *    a shaped frame, an FCS trial passes with 2^-16 and the address check passes a random field with about (37/256)^12.
 *  - Selection: only plain and repaired candidates count.  The first opens a group; those less than 8 slots (one bit: the neighbouring phases of one
 *    frame) behind it contest the delivery -- fewest flips, then the largest metric (the sum of |d| over the walked bits, uint64), then the lowest
 *    slot -- and the winner is delivered once every slot of the contest is decided.  A later passing candidate whose slot lies more than 8 slots
 *    in front of the delivered frame's closing-flag slot is an overlap: dropped, overlaps += 1.  A closing flag shared with the next frame is a
 *    candidate like any other.  Frames wait on the host, per stream in increasing position, until hd_afsk_take_frames.
 *  - Counters per stream: samples, slots, flags (candidates decided), unshaped (abort, open or not shaped), fcs_failures, frames_plain,
 *    frames_repaired, refused (address check), overlaps; the modem's integers F, W, step[2].
 *  - Queue, errors: as the clocked decoder's; a push returns when its kernels are done.  A push longer than max_push: HD_ERR_CAPACITY.  A row longer
 *    than HD_AFSK_CHUNK samples is cut into launches; a scan's candidates into launches of at most HD_AFSK_LAUNCH over all streams.  The slot ring must
 *    hold the longest walk on all phases, the gate's look back and a push: 8 L + 72 + max_push <= HD_AFSK_RING, or create refuses (HD_ERR_UNSUPPORTED).
 *  - Not built: a band-pass or de-emphasis stage in front of the tone pair (a DC offset on the row leaks into the space filter with a weight of about
 *    0.09, NOTES.md); several slicers with different space gains; 9600 baud G3RUH; connected-mode AX.25; parsing of APRS position formats. */
#define HD_AFSK_MAX_SPB 2048
#define HD_AFSK_CHUNK 4096         /* samples of a row per launch of the slot kernel */
#define HD_AFSK_LAUNCH 4096        /* candidates per launch of the frame kernel over all streams */
#define HD_AFSK_RING 65536         /* slots of a stream's ring */
#define HD_AFSK_MAX_FRAME 332      /* bytes, FCS included */
#define HD_AFSK_MIN_FRAME 17
#define HD_AFSK_OPEN 0             /* hd_afsk_candidate.result */
#define HD_AFSK_ABORT 1
#define HD_AFSK_UNSHAPED 2
#define HD_AFSK_FCS_FAILED 3
#define HD_AFSK_REFUSED 4
#define HD_AFSK_PLAIN 5
#define HD_AFSK_REPAIRED 6
typedef struct hd_afsk hd_afsk;
typedef struct hd_afsk_params {
    uint32_t max_push;         /* longest push per stream in samples; 0: what the engine's longest call leaves, or 4096 */
    uint32_t max_frame_bytes;  /* HD_AFSK_MIN_FRAME .. HD_AFSK_MAX_FRAME, FCS included; default 332 */
    uint32_t repair_bits;      /* default 8 */
    uint32_t repair_flips;     /* 0 .. 4; default 2 */
    uint32_t require_addr;     /* default 1 */
    uint32_t _pad;
} hd_afsk_params;
typedef struct hd_afsk_rx {    /* one delivered frame */
    uint64_t slot;             /* the slot of the opening flag's last bit, 8 k + phase */
    uint64_t start_sample;     /* the first sample behind that bit: (slot + 8) F >> 19 */
    uint64_t close_slot;       /* the slot of the closing flag's last bit */
    uint64_t metric;
    uint32_t len;              /* bytes of data */
    uint32_t flips, phase, addr_ok, fcs, _pad;
    uint8_t  data[HD_AFSK_MAX_FRAME];   /* the frame without its FCS */
    uint32_t _pad2;
} hd_afsk_rx;
typedef struct hd_afsk_candidate {   /* one candidate, whatever became of it (the frame kernel's, the restatement's and the test hooks' record) */
    uint64_t slot, close_slot /* 0 unless closed */, metric;
    uint32_t result;           /* HD_AFSK_OPEN .. HD_AFSK_REPAIRED */
    uint32_t bits;             /* the bits the hard walk took */
    uint32_t len;              /* the frame's bytes, FCS included; 0 unless shaped */
    uint32_t flips, addr_ok, fcs;
    uint8_t  data[HD_AFSK_MAX_FRAME];   /* the frame with its FCS: the winning pattern's, the hard walk's where none won */
    uint32_t _pad;
} hd_afsk_candidate;
typedef struct hd_afsk_counters {
    uint64_t samples, slots, flags, unshaped, fcs_failures, frames_plain, frames_repaired, refused, overlaps;
    uint32_t F, W, step[2];    /* the modem's integers: F = 0, no modem */
} hd_afsk_counters;
void hd_afsk_params_default(hd_afsk_params* p);
/* HD_ERR_INVALID: max_frame_bytes, repair_flips, more than 64 flip patterns; HD_ERR_UNSUPPORTED: the ring does not hold 8 L + 72 + max_push slots,
 * more than HD_AFSK_LAUNCH streams. */
int  hd_afsk_create(hd_engine* e, const hd_afsk_params* p /* null: the defaults */, hd_afsk** out);
void hd_afsk_destroy(hd_afsk* a);
/* Samples, slots, candidates, counters and the open group of the stream start again; the modem stays, and so do frames not yet taken. */
int  hd_afsk_reset(hd_afsk* a, uint32_t stream /* UINT32_MAX: all */);
int  hd_afsk_set_modem(hd_afsk* a, uint32_t stream, double baud, double mark_hz, double space_hz);   /* resets the stream */
int  hd_afsk_set_bell202(hd_afsk* a, uint32_t stream);                                               /* 1200 baud, 1200 / 2200 Hz */
/* The three doors of the clocked decoder, with its rules; each ends with a scan. */
int  hd_afsk_push_engine(hd_afsk* a);
int  hd_afsk_push_device(hd_afsk* a, const float* d_rows, size_t stride, const uint32_t* n_per_stream, uint32_t n);
int  hd_afsk_push_host(hd_afsk* a, const float* rows, size_t stride, const uint32_t* n_per_stream, uint32_t n);
/* Hands out up to cap of the stream's waiting frames, oldest first, and returns how many were written; out null: how many wait.  Negative: HD_ERR_*. */
int  hd_afsk_take_frames(hd_afsk* a, uint32_t stream, hd_afsk_rx* out, size_t cap);
int  hd_afsk_stats(hd_afsk* a, uint32_t stream, hd_afsk_counters* out);

#ifdef __cplusplus
}
#endif
#endif /* HABDEC_AMD_H */
