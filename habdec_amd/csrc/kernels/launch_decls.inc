// Launchers of the kernels whose FIR arithmetic depends on the engine's mode (hd_engine_config.arith): declared once per mode namespace by launch.h --
// hd::exact (separately rounded multiply and add, ascending tap order: bit-identical to the reference's CPU arithmetic) and hd::fast (fused multiply-add,
// tolerance 1e-5: arith.h).  Defined in decimate.hip, fir_demod.hip and tail.hip, each compiled once per mode (build.py).
// One FIR-decimate stage for all streams.  `final_stage`: output lands behind the FIR history in the
// low-pass input buffer (offset fir_hist_cap + pend_before), else at offset 0 of `out`.
// Returns false when (ratio, ntaps) is not one of the eight reference designs.  The kernel also carries each
// stream's last ntaps-1 inputs into `hist_out` (Decimator.h:140-143, incl. the in-place quirk Q4); hist_in/hist_out
// are ping-ponged by the caller.
bool launch_decimate(hipStream_t st, int ratio, int ntaps, uint32_t n_streams, uint32_t max_out,
                     const float2* in, size_t in_stride, const float2* hist_in, float2* hist_out, const float* taps,
                     float2* out, size_t out_stride, const StreamCall* call, int stage, int final_stage,
                     uint32_t fir_hist_cap, float2* fft_in /* final stage: spectrum input buffer [S][4096], or null */,
                     uint32_t lin_wgs = 0 /* != 0: every stream has the same size; use exactly this many workgroups (single-wave kernels) */);
// The same stage as the FIRST stage of a call in which some stream is tuned at the input rate (hd_stream_set_front_tune): sample i of stream s's input is
// rotated by theta = Pf + i Df on its way into the tile, ftune[s] = (Df, Pf) read in place (mapped host memory), ftab = the phasor tables [C | F] of
// tune.h in device memory; the history carry holds rotated samples.  A stream with Df = Pf = 0 is computed exactly as by launch_decimate.
bool launch_decimate_tuned(hipStream_t st, int ratio, int ntaps, uint32_t n_streams, uint32_t max_out,
                           const float2* in, size_t in_stride, const float2* hist_in, float2* hist_out, const float* taps,
                           float2* out, size_t out_stride, const StreamCall* call, int final_stage,
                           uint32_t fir_hist_cap, float2* fft_in, uint32_t lin_wgs, const uint2* ftune, const float* ftab);
// copy `bytes` (multiple of 16) from mapped pinned host memory into device memory with a kernel
void launch_fetch_params(hipStream_t st, const void* host_mapped, void* dst, size_t bytes);
// factor 1: copy the chunk behind the FIR history.
void launch_passthrough(hipStream_t st, uint32_t n_streams, uint32_t max_n, const float2* in, size_t in_stride,
                        float2* out, size_t out_stride, const StreamCall* call, uint32_t fir_hist_cap);
// The per-chunk post-pass of the separate-kernels path: the DC blocker where StreamCall::dc_remove asks for it, then the rotation of a tuned stream
// (tune.h; tune[s] = (step, phase), tune = null: no stream of the call is tuned), in place on the decimated chunk behind the FIR history.
void launch_chunk_post(hipStream_t st, uint32_t n_streams, float2* fbuf, size_t stride, const StreamCall* call, uint32_t fir_hist_cap,
                       const uint2* tune, const float* tune_tab);
void launch_fft_feed(hipStream_t st, uint32_t n_streams, const float2* fbuf, size_t stride, float2* fft_in,
                     const StreamCall* call, uint32_t fir_hist_cap);
// (max_taps sizes the tile's LDS image, host/fir_lds.hpp: fir_demod_lds_bytes; false, and nothing launched, when it and the kernel's static LDS exceed lds_limit
// -- what the device grants a workgroup -- or the opt-in above 64 KB fails)
bool launch_fir_demod(hipStream_t st, uint32_t n_streams, uint32_t max_m, uint32_t max_taps, size_t lds_limit, const float2* fbuf, size_t stride,
                      const float* taps, uint32_t taps_stride, float* demod, size_t demod_stride, float2* filtered /*or null*/,
                      const DemodCarry* carry_in, DemodCarry* carry_out, const StreamCall* call, uint32_t fir_hist_cap,
                      float* sym_ring, uint32_t ring_cap, const SymState* sym, float2* fbuf_next,
                      float2* head_side /* [S][head_cap] */, uint32_t head_cap, const float2* fbuf_prev /* the previous call's low-pass buffers: FirHistory, dev_types.h */,
                      uint32_t* ck_acc = nullptr /* [S][2], zero before the launch: the call's discriminator checksum accumulates here (BitsHeader::demod_ck; launch_symbols collects it) */,
                      const float2* pre = nullptr /* the low-pass output computed through transforms (below), [S][pre_stride] x pre_scale: the kernel then does everything but the filter */,
                      uint32_t pre_stride = 0, float pre_scale = 1.0f,
                      const uint32_t* pre_flags = nullptr /* with `pre`: the flags launch_lp_gather left -- a stream whose block held a zero sample in the call `pre_tag` is summed directly */,
                      uint32_t pre_tag = 0);
// The transform route of a long low-pass (fast mode): input image [history | inputs | zeros] of N per stream, the taps' image, the product of the spectra
// X conj(K); rocFFT runs between them (engine.cpp)
void launch_lp_gather(hipStream_t st, uint32_t n_streams, const float2* fbuf, size_t stride, float2* work, uint32_t N, const StreamCall* call, uint32_t fir_hist_cap,
                      const float2* head_side, uint32_t head_cap, const float2* fbuf_prev, uint32_t* flags /* [S][2] */, uint32_t tag);
void launch_lp_taps_gather(hipStream_t st, uint32_t n_streams, const float* taps, uint32_t taps_stride, const uint32_t* ntaps, float2* kf, uint32_t N);
void launch_lp_mul(hipStream_t st, uint32_t n_streams, float2* work, const float2* kf, uint32_t N, const StreamCall* call);
// Fills the LDS carve for `lanes` (64 or 256) lanes per stream; returns false when (ratio2, ntaps2) has no tail instantiation or the
// windows for max_taps / max_R do not fit into lds_limit bytes -- the caller then runs launch_decimate + launch_fir_demod
// and launch_symbols instead.
bool tail_layout(TailArgs& a, int lanes, int ratio2, int ntaps2, uint32_t max_taps, uint32_t max_R, uint32_t min_R, uint32_t ring_cap,
                 uint32_t pend_max /* most pending samples any stream has in front of or behind this call's low-pass run */, uint32_t lds_limit,
                 int op = 0 /* stage-2 outputs per lane and piece: 0 = the default of `lanes` (4 for 64 lanes, 1 for 256); 256 lanes also take 4 */);
bool launch_tail(hipStream_t st, int lanes, int ratio2, int ntaps2, uint32_t n_streams, const TailArgs& a, hipEvent_t ev_stop = nullptr);
// Batch mode, two-stage plans whose first stage is a single-wave design: ONE launch per step -- the stream tails of the previous call
// (workgroups [0, n_tail), arguments `ta`) in front of this call's stage 1 as a linear split over stage1_wgs workgroups; every stream
// has n_out stage-1 outputs.  Returns false when there is no instantiation for the plan.
bool launch_step(hipStream_t st, int ratio, int ntaps, int ratio2, int ntaps2, uint32_t n_streams, uint32_t n_out, const float2* in, size_t in_stride,
                 const float2* hist_in, float2* hist_out, const float* taps, float2* out, size_t out_stride, const StreamCall* call,
                 StreamCall* call_copy, uint32_t stage1_wgs, const TailArgs& ta, uint32_t n_tail,
                 uint32_t uniform_n /* != 0: the streams' common sample count, and no stream restarts its stage-1 history this call */,
                 const StepClaim& claim = StepClaim{});
// The same step as ONE 512-thread workgroup per CU (k_step_cu, decimate.hip): four stage-1 worker waves (stage1_ring.h: ring_worker -- LDS-DMA into the
// wave's own slot, systolic tap loop) and the tails in the other four waves, which become workers when they are done.  Needs a /32 first stage, equally
// sized pushes that are a multiple of 2048 samples, drawn runs (claim.ctr) and no history restart; returns false otherwise (the caller then launches
// k_step).  tail_bytes: LDS slice of one tail (<= step_cu_tail_lds).
bool launch_step_cu(hipStream_t st, int ratio, int ntaps, int ratio2, int ntaps2, uint32_t n_streams, uint32_t n_cus, const float2* in, size_t in_stride,
                    const float2* hist_in, float2* hist_out, const float* taps, float2* out, size_t out_stride, const StreamCall* call,
                    StreamCall* call_copy, const TailArgs& ta, uint32_t n_tail, uint32_t uniform_n, const StepClaim& claim, uint32_t tail_bytes,
                    hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr /* signalled by the dispatch itself (hipExtLaunchKernel), not by a packet behind it */);
uint32_t ring_tiles(int ratio, int ntaps, uint32_t n);   // tiles per stream and call of the per-CU ring kernels for n input samples (0: none); the drawn runs must divide it
bool step_cu_supported(int ratio, int ntaps, int ratio2, int ntaps2);   // plans k_step_cu is instantiated for: /64 (/32 212 + /2 69), /128 (/32 174 + /4 139)
bool stage1_cu_supported(int ratio, int ntaps);   // stages k_stage1_cu exists for: /32 (212, 174 taps), /8 (54 taps) as first stages; /4 (139 taps) as the only stage of a plan
// Stage 1 alone in the same shape (eight tile slots by default; two loader and six computing waves at /8, one and fifteen at /4, worker waves at /32 and /64): a /32, /64 or /8 first stage or /4 as the only one,
// equally sized pushes that are a multiple of 2048 samples, drawn runs, no history restart; false otherwise (the caller then launches k_decimate).  The call's parameter block is not copied.
bool launch_stage1_cu(hipStream_t st, int ratio, int ntaps, uint32_t n_cus, const float2* in, size_t in_stride, const float2* hist_in, float2* hist_out,
                      const float* taps, float2* out, size_t out_stride, uint32_t uniform_n, const StepClaim& claim, unsigned int* gave_up,
                      uint32_t n_slots = 8 /* tile slots (2 per loader .. 8): fewer leave LDS for the other queue's kernels */,
                      const StreamCall* final_call = nullptr /* /4 only: the stage is the final one of a single-stage plan -- per-stream pend_before / fft_take / fft_fill */,
                      uint32_t fir_hist_cap = 0, float2* fft_in = nullptr);
uint32_t step_cu_tail_lds(int ratio, int ntaps);   // LDS a tail may use inside k_step_cu beside the four worker slots of that first stage; 0 = no such kernel
uint32_t probe_xcc_mask(hipStream_t st, uint32_t n_cus, unsigned int* d_word);   // bit x set = some workgroup of a chip-filling grid ran on XCC id x
uint32_t step_lds_bytes(int ratio, int ntaps);   // LDS of a step-launch workgroup for that first stage (its tile, at least kStepLdsBytes); 0 = no step kernel
// Symbol extractor: window kernel over the positions that became computable (at most max_new per stream) + scan kernel.
void launch_symbols(hipStream_t st, uint32_t n_streams, uint32_t max_m, uint32_t max_new, uint32_t max_R, const float* tail,
                    uint32_t ring_cap, SymState* sym, unsigned long long* flipmask, float* weight, const SymbolParams* sp,
                    const StreamCall* call, uint32_t* slots, uint32_t slot_words, uint32_t* flips_dbg, uint32_t flips_cap,
                    uint32_t min_R /* smallest averaging half-window over the streams: bounds the flips one call can find */,
                    uint32_t seq /* the call's tag, stored last into every result slot (BitsHeader::seq) */,
                    hipEvent_t ev_stop = nullptr /* signalled by the dispatch itself, as in launch_step_cu */,
                    uint32_t* ck_acc = nullptr /* the sums launch_fir_demod left for this call: into the result slot's demod_ck / demod_n, then cleared */);
