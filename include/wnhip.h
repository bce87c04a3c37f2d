/*
 * wnhip.h — C ABI of libwnhip.so, the MI355X (gfx950) generation engine that
 * replaces the TensorFlow graph execution on the generation path of
 * bfs18/nsynth_wavenet.
 *
 * The reference exposes NO native/FFI interface for this path (it is pure
 * Python over TensorFlow 1.x).  Its seam is Python:
 *     wavenet/parallelgen.py:22   synthesis(hparams, mel, save_paths, checkpoint_path)
 *     wavenet/fastgen.py:69       encode(hparams, wav_data, checkpoint_path)
 *     wavenet/fastgen.py:128      synthesis(hparams, mel_encoding, save_paths, checkpoint_path)
 * and inside those, one `sess.run` on the graphs built by
 *     wavenet/parallel_wavenet.py:289-359   ParallelWavenet.feed_forward + _clip_quant_scale
 *     wavenet/wavenet.py:142-155            Wavenet.deconv_stack
 *     wavenet/wavenet.py:379-514            Fastgen.sample
 * Each entry point below states which of those `sess.run` calls it replaces.
 * The ctypes binding a maintainer of the reference would add is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - Plain C, no torch / HIP types in signatures: a stream is passed as the
 *     raw hipStream_t value in a `void*` (NULL = the null stream).
 *   - Every pointer is a DEVICE pointer unless its name ends in `_host`.
 *   - The caller owns every input, output and workspace buffer; the library
 *     owns only the handle and its packed weights.  No allocation and no host
 *     synchronisation happens inside the generate calls (wn_ar_generate, whose
 *     sample loop is driven from the host, is the documented exception: it
 *     enqueues work and returns without synchronising, but it instantiates a
 *     hipGraph).
 *   - Return value: 0 on success, a negative errno-style code otherwise
 *     (WN_EINVAL shape/config, WN_ENOENT unknown/missing weight, WN_ENOMEM
 *     workspace too small, WN_EIO HIP runtime error, WN_ESTATE wrong call
 *     order).  Nothing throws or aborts across the ABI; the message is
 *     available from wn_last_error().
 *   - Concurrency (SURVEY 8(b) "Threading / streams"; tests/test_gpu_threads.py drives one handle from two
 *     host threads on two streams).  After wn_finalize() the weights and every table of a handle are read-only.
 *     The WORK calls -- wn_deconv, wn_iaf_generate*, wn_iaf_encode, wn_iaf_latent_log_prob, wn_iaf_range_*, wn_clip_quant, wn_ar_reset / wn_ar_step /
 *     wn_ar_generate / wn_ar_cond_vars, wn_teacher_forward / wn_teacher_log_prob / wn_teacher_log_prob_grad, wn_distill_mol_xent /
 *     wn_distill_gauss_kl -- keep all per-call state (the
 *     range-guard word, the autoregressive queues and step counter) in the caller's workspace / state buffer:
 *     any number of host threads may issue them on ONE handle at the same time, each with its own workspace
 *     and stream.  (wn_ar_generate's hipGraphs are per call; the handle only keeps them alive until their
 *     stream has run them.)
 *     The SWITCHES -- wn_iaf_set_groups, wn_ar_set_graph, wn_profile_begin / _pause / _end,
 *     wn_profile_parts_begin / _only / _end -- change how later work calls of the handle run.  They take the
 *     handle exclusively: while a work call of another thread is inside the library they return WN_ESTATE
 *     ("busy") and change nothing; a work call reads every switch once, at its entry.  The two measurement
 *     modes (wn_profile_*) are for single-caller benchmarking: with several callers the recorded events
 *     interleave (the lists themselves are locked).
 *     wn_last_error() returns the message of the CALLING THREAD's last failed call.
 */
#ifndef WNHIP_H_
#define WNHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WN_ABI_VERSION 1

/* libwnhip.so is linked with -fvisibility=hidden: the functions declared here are its whole dynamic symbol table
 * (tests/test_host.py checks `nm -D --defined-only` against this header, both ways). */
#define WN_API __attribute__((visibility("default")))

#define WN_OK       0
#define WN_EINVAL  (-22)
#define WN_ENOENT  (-2)
#define WN_ENOMEM  (-12)
#define WN_EIO     (-5)
#define WN_ESTATE  (-1)
#define WN_ERANGE  (-34)   /* wn_iaf_range_status: an activation left the fp16 range of the split-fp16 arithmetic */

/* `form` of wn_iaf_generate_form / wn_iaf_workspace_bytes_form: which arithmetic ONE call runs in */
#define WN_FORM_DEFAULT     (-1)  /* what the handle was created for (wn_config.precision / cond_mode) */
#define WN_FORM_F16X3        0    /* split-fp16 MFMA, conditioning placed by the handle's cond_mode policy */
#define WN_FORM_F32          1    /* fp32 MFMA (the reference's own arithmetic): no fp16 range limit, ~2.3x slower */
#define WN_FORM_F16X3_FUSED  2    /* split-fp16 MFMA without the hoisted-conditioning workspace */

#define WN_MAX_DECONV 4
#define WN_MAX_FLOWS  8

/* kind */
#define WN_KIND_STUDENT 0   /* ParallelWavenet (IAF), parallel_wavenet.py */
#define WN_KIND_TEACHER 1   /* Wavenet / Fastgen (autoregressive), wavenet.py */
/* loss_type */
#define WN_LOSS_CE       0
#define WN_LOSS_MOL      1
#define WN_LOSS_GAUSS    2
#define WN_LOSS_LOGISTIC 3  /* student only: noise source (parallel_wavenet.py:303-306) */
/* upsample_act (masked.py:28-36) */
#define WN_ACT_TANH       0
#define WN_ACT_RELU       1
#define WN_ACT_LEAKY_RELU 2 /* alpha = 0.4 */

/* Plain-C mirror of the config JSON (config_jsons/NAME.json) after the
 * reference's per-class getattr defaults have been applied by the caller
 * (wavenet.py:105-129,326-345; parallel_wavenet.py:124-141). */
typedef struct wn_config {
    int32_t kind;
    int32_t n_mel;                          /* 80 (mel_extractor.py:17) */
    int32_t width;                          /* residual channels */
    int32_t skip_width;                     /* teacher only */
    int32_t gate_width;                     /* student: width; teacher: width or 2*width */
    int32_t deconv_width;
    int32_t n_deconv;                       /* len(deconv_config) */
    int32_t deconv_filter[WN_MAX_DECONV];
    int32_t deconv_stride[WN_MAX_DECONV];
    int32_t filter_length;                  /* 3 (masked.py:349 asserts it) */
    int32_t num_stages;
    int32_t num_layers;                     /* teacher */
    int32_t n_flows;                        /* student: len(num_iaf_layers) */
    int32_t iaf_layers[WN_MAX_FLOWS];
    int32_t use_mu_law;
    int32_t loss_type;
    int32_t mol_mix;
    int32_t out_width;                      /* teacher: 256/65536 (ce), 3*mol_mix, 2; student: 2 */
    int32_t share_deconv;                   /* use_share_deconv || use_teacher_deconv */
    int32_t use_weight_norm;
    int32_t upsample_act;
    int32_t precision;                      /* IAF / upsampler contractions: 0 split-fp16 x3 on the
                                               fp16 MFMA (default), 1 fp32 MFMA */
    int32_t cond_mode;                      /* where the split-fp16 path evaluates the per-layer
                                               conditioning 1x1s: 0 default (= 2 unless the
                                               environment says WN_COND=fused or the projected term
                                               of the call would exceed a third of the device memory
                                               / half of what was free at wn_create), 1 inside every
                                               layer kernel, 2 one GEMM per deconv stack */
    int32_t use_resize_conv;                /* upsampler = nearest-neighbour resize + SAME conv
                                               (masked.py:294-322) instead of transposed conv;
                                               variables <prefix>resize_conv_i/{W,biases} */
    int32_t reserved[5];                    /* must be 0 */
} wn_config;

typedef struct wn_handle wn_handle;

WN_API int wn_abi_version(void);

/* Build an empty engine for one model on the current HIP device.
 * Replaces graph construction (parallelgen.py:11-19, fastgen.py:61-66,118-125).
 * Students of the shipped shape (width 64, deconv_width 256, num_stages >= 7) run on the MFMA kernels; any other even
 * width <= 416 (one tile of the generic layer kernel must fit the 160 KB of LDS) / deconv_width % 64 == 0 /
 * num_stages >= 3 on generic fp32 kernels (same results, much slower).
 * Teachers: 3 * width + deconv_width <= 2048 runs on the tuned step kernels (every shipped wavenet_*.json), up to 4096 on
 * a wide instantiation of the same kernels (a correctness path: below four utterances, and at every batch size when
 * 3*width + deconv_width + gate_width/2 > 3072, one utterance at a time; otherwise the batched step); beyond that wn_create refuses. */
WN_API int wn_create(const wn_config* cfg_host, wn_handle** out);

/* Provide one variable under its TensorFlow name WITHOUT the
 * '/ExponentialMovingAverage' suffix and ':0' (fastgen.py:12-14), in the
 * reference's shape: conv kernels HWIO [1,K,Cin,Cout] '<scope>/W', biases
 * '<scope>/biases' (masked.py:190-200); transposed-conv kernels [1,K,Cout,Cin]
 * '<scope>/kernel', '<scope>/bias' (masked.py:249-260); weight-norm pairs
 * '<name>_V','<name>_g' (masked.py:145-153).  Replaces Saver.restore
 * (parallelgen.py:29-41, fastgen.py:80-84,142-147).  Unknown names -> WN_ENOENT. */
WN_API int wn_set_weight(wn_handle* h, const char* tf_var_name,
                  const float* data_host, const int64_t* shape_host, int rank);

/* Check that every variable the config needs is present, fold weight-norm
 * (W = V/||V||*g), repack into the kernels' MFMA-fragment order, upload. */
WN_API int wn_finalize(wn_handle* h);

/* Length helpers: samples produced for F mel frames.
 *   IAF:  T  = (F*frame_shift // 2^(num_stages-1)) * 2^(num_stages-1)  (parallel_wavenet.py:293-302)
 *   AR :  Tn = F*frame_shift                                          (fastgen.py:136,156)      */
WN_API int64_t wn_iaf_length(const wn_handle* h, int F);
WN_API int64_t wn_ar_length(const wn_handle* h, int F);

/* Bytes of caller-provided scratch needed by wn_deconv / wn_iaf_generate /
 * wn_ar_generate for batch B and F frames (Tn = wn_ar_length for AR).
 * The first 256 bytes of a workspace hold the range-guard words of the generate calls made on it
 * (wn_iaf_range_status*); every call -- wn_deconv included -- leaves them to those functions, so one buffer can
 * serve wn_iaf_generate and wn_deconv in any order. */
WN_API size_t wn_workspace_bytes(const wn_handle* h, int B, int F);

/* Wavenet.deconv_stack (wavenet.py:46-73,142-155): mel [B,F,n_mel] ->
 * enc [B, F*frame_shift, deconv_width] in the REFERENCE layout (time-major),
 * i.e. what fastgen.encode returns (fastgen.py:69-88).  `scope` is the
 * variable-name prefix: "" (teacher), "iaf_share", "iaf_1", ... */
WN_API int wn_deconv(wn_handle* h, const char* scope, const float* mel, int B, int F,
              float* enc, void* ws, size_t ws_bytes, void* stream);

/* Which kernels the upsampler stack `scope` runs for batch B and F frames, one entry per layer in order, joined by ", ":
 * the GEMM form -- front (deconv_front_kernel), pg (deconv_pg_kernel), hs<T> (deconv_mfma_hs_kernel<TAPS>), h<false|true>
 * (deconv_mfma_h_kernel<G4IN>), fa (the frame-axis fp32 GEMM), mfma (deconv_mfma_kernel) -- then, where a weave launch
 * follows it, il (deconv_interleave_kernel) or g4<S> (deconv_interleave_g4_kernel<S>): "front, pg", "h<false> g4<10>, hs<4> il".
 * split_out 0: fp32 rows out, as wn_deconv; 1: G4 words out, as the generate, teacher and training calls ask for.
 * precision: -1 = the handle's, else a value of wn_config.precision (the arithmetic of one call, as WN_FORM_F32 selects it).
 * Launches nothing and needs no workspace.  WN_ESTATE / WN_ENOENT as wn_deconv; WN_EINVAL for a null or short buffer. */
WN_API int wn_deconv_forms(const wn_handle* h, const char* scope, int B, int F, int split_out, int precision, char* buf,
                           size_t cap);

/* The single sess.run of parallelgen.synthesis (parallelgen.py:43-45):
 * ParallelWavenet.feed_forward (parallel_wavenet.py:289-345) followed by
 * _clip_quant_scale (:347-359).
 *   mel        [B,F,n_mel]
 *   noise      [B,T] injected logistic/normal draws, or NULL -> drawn on the
 *              device from `seed` (Philox4x32-10; logistic via log u - log(1-u),
 *              u ~ U(1e-5,1-1e-5), or N(0,1) for loss_type gauss)
 *   wav        [B,T]  float32 on the 2/Q grid (or the inverse-mu-law table)
 *   idx        [B,T]  int32 quantisation index in [-Q/2,Q/2)        (optional)
 *   x_raw      [B,T]  feed_forward's 'x' before clipping           (optional)
 *   mean_tot, scale_tot [B,T] as returned by feed_forward          (optional)
 *   rand_out   [B,T]  the noise actually used ('rand_input')       (optional) */
WN_API int wn_iaf_generate(wn_handle* h, const float* mel, int B, int F,
                    const float* noise, uint64_t seed,
                    float* wav, int32_t* idx, float* x_raw,
                    float* mean_tot, float* scale_tot, float* rand_out,
                    void* ws, size_t ws_bytes, void* stream);

/* The same call in an explicitly named arithmetic (every student handle carries the weights in both packings), and
 * its workspace size.  wn_iaf_generate(h, ...) == wn_iaf_generate_form(h, WN_FORM_DEFAULT, ...); wn_workspace_bytes
 * (default form) also covers WN_FORM_F32 and WN_FORM_F16X3_FUSED, so a re-run never needs a larger workspace.
 *
 * fp16 range guard.  The split-fp16 forms carry activations as fp16 hi+lo pairs: 22-bit significand, but the fp16
 * EXPONENT range -- |value| >= 65504 would become inf where the reference's fp32 graph is still finite (scale may reach
 * e^7 per flow, parallel_wavenet.py:105-114).  Every kernel that produces such pairs (upsampler, start conv, residual
 * layers) checks the magnitudes it converts and raises a status word at the head of the call's workspace; the call then
 * writes NaN to every float output (idx = 0) instead of audio computed from saturated operands.  The generate call
 * itself stays asynchronous; wn_iaf_range_status(h, ws, stream) SYNCHRONISES the stream, reads that word and returns
 * WN_OK or WN_ERANGE -- on WN_ERANGE re-run the call with wn_iaf_generate_form(h, WN_FORM_F32, ...) (same workspace).
 * The Python Engine does exactly that by itself (Engine.iaf_generate(check_range=True), the default).  Never silent. */
WN_API int wn_iaf_generate_form(wn_handle* h, int form, const float* mel, int B, int F,
                         const float* noise, uint64_t seed,
                         float* wav, int32_t* idx, float* x_raw,
                         float* mean_tot, float* scale_tot, float* rand_out,
                         void* ws, size_t ws_bytes, void* stream);
WN_API size_t wn_iaf_workspace_bytes_form(const wn_handle* h, int form, int B, int F);
WN_API int wn_iaf_range_status(wn_handle* h, const void* ws, void* stream);
/* A run of calls kept asynchronous (a serving or timing loop that does not want one host synchronisation per call):
 * the second word of the workspace head accumulates the status words of every call made on that workspace.
 * wn_iaf_range_reset(h, ws, stream) zeroes the 64-byte head (do it once for a fresh workspace and before a run);
 * wn_iaf_range_status_since_reset(h, ws, stream) SYNCHRONISES, returns WN_ERANGE if ANY call since the reset left the
 * fp16 range (each such call NaN-poisoned its own outputs, as above) and resets.  Both touch only the workspace. */
WN_API int wn_iaf_range_reset(wn_handle* h, void* ws, void* stream);
WN_API int wn_iaf_range_status_since_reset(wn_handle* h, void* ws, void* stream);

/* Windowed generation: utterances of any length as a batch of windows.
 *
 * Geometry a planner needs: `reach` = samples to the left of t that sample t depends on (sum over the flows of
 * filter_length + (filter_length - 1) sum of the flow's dilations; 12 288 for the shipped configs); frames_before /
 * frames_after = mel frames left / right of the frame holding an upsampled column that reach that column through the
 * deconv stack; period = max_dilation / gcd(frame_shift, max_dilation): the centre crop of a call on F frames depends on
 * F modulo it.  Any output pointer may be NULL.  nsynth_wavenet_amd.config.iaf_plan_windows is a planner on top of it. */
WN_API int wn_iaf_window_geometry(const wn_handle* h, int64_t* reach, int* frames_before, int* frames_after, int* period);

/* One row of a window call: an ordinary row of T_w = wn_iaf_length(h, Fw) samples whose local sample t is sample
 * t_origin + t of utterance b; of these the local range [keep_from, keep_to) is written, to out[b][out_t ..]. */
typedef struct wn_iaf_window_row {
    int32_t b;
    int64_t t_origin, keep_from, keep_to, out_t;
} wn_iaf_window_row;

/* wn_iaf_generate_form on R rows of Fw frames (mel [R,Fw,n_mel], each row in the natural layout of a call on Fw frames)
 * with two differences.  The noise of row r is the noise of utterance b at t_origin + t: drawn from `seed` with the
 * counter of a one-shot call at that position (a row with b = r, t_origin = 0 gets the one-shot's bits), or read from
 * noise_abs [B_out,T_out] (0 outside [0, T_out)).  And only the kept samples leave, into COMPACT outputs
 * wav, idx, x_raw, mean_tot, scale_tot, rand_out [B_out,T_out] (all but wav optional).  rows_host is a HOST array; the
 * call copies it.  Refused with WN_EINVAL: everything wn_iaf_generate_form refuses; b outside [0, B_out); a t_origin
 * that is negative or not a multiple of 4; a kept range outside [0, T_w); out_t plus the kept length past T_out; kept
 * ranges of two rows that overlap in the output.  The 2,000,000-sample limit applies to Fw frame_shift.  Whether the
 * residual layers run as layer groups is the one-shot's policy for a batch of form_rows rows (0: R); with a fixed
 * form_rows a row's result does not depend on how many rows share its call.  The range guard
 * and wn_iaf_range_status* work as for the one-shot call: a fault in any row makes every kept sample of the call NaN. */
WN_API int wn_iaf_generate_windows(wn_handle* h, int form, int form_rows, const float* mel, int R, int Fw,
                            const wn_iaf_window_row* rows_host, const float* noise_abs, int B_out, int64_t T_out,
                            uint64_t seed, float* wav, int32_t* idx, float* x_raw,
                            float* mean_tot, float* scale_tot, float* rand_out,
                            void* ws, size_t ws_bytes, void* stream);
/* wn_iaf_workspace_bytes_form(h, form, R, Fw) plus the row table (0 for a bad argument) */
WN_API size_t wn_iaf_windows_workspace_bytes(const wn_handle* h, int R, int Fw, int form);

/* The inverse of the student: the latent z with feed_forward(noise = z)['x'] == x, by fixed-point sweeps.
 * feed_forward returns x = z scale_tot(z) + mean_tot(z) where scale_tot[t], mean_tot[t] depend on z[< t] only, so
 * z <- (x - mean_tot(z)) / scale_tot(z) is exact on the first k samples after k sweeps.  One call enqueues n_sweeps sweeps on
 * `stream` without a host synchronisation; a sweep is the prologue with noise = z, the residual stack of the generate
 * call, and a back kernel: z' = (x - mean_tot) / min(scale_tot, e^7), a non-finite z' becomes 0, then z' is clamped to
 * +-z_max; z [B,T] is read and written in place.
 *   x, z                 [B,T]  T = wn_iaf_length(h, F); z holds the starting iterate on entry
 *   tol                  front[b] = the smallest t with |z' - z| > tol in the LAST sweep of the call, T if none (int32 [B]);
 *                        tol = 0 compares the bits
 *   mean_tot, scale_tot  [B,T] of the last sweep's input iterate -- the converged z's own once front == T   (optional)
 *   counts               int32 [4]: [0] elements clamped in the last sweep; [1] the OR of the range words of the call's
 *                        sweeps (non-zero: a split-fp16 operand left the fp16 range; such a sweep leaves z as it was and
 *                        writes NaN to mean_tot / scale_tot -- go on from the same z with WN_FORM_F32 and first = 1);
 *                        [2] the first sweep of this call, counted from 1, after which every front was T and nothing was
 *                        clamped, 0 if none -- the call's later sweeps then change nothing, so z, the totals and front
 *                        are that sweep's; [3] 0.  The workspace's accumulated status word is left alone.
 *   first                1: the call computes the upsampler and the conditioning term (a fresh encode, a new mel, another
 *                        form, another workspace).  0: CALLER CONTRACT -- the previous call on this workspace was a
 *                        wn_iaf_encode of the same handle, form, mel contents, B and F, and nothing has written the
 *                        workspace since; a student with a shared deconv stack then reuses the encoding and the
 *                        conditioning term that call left there and runs neither the upsampler nor the conditioning GEMM.
 *                        Within one call only the first sweep runs them in any case.  Students with private stacks run
 *                        both in every sweep whatever `first` says.
 * Refused with WN_EINVAL: a teacher handle; a mu-law student (its x is not the flow's output); n_sweeps < 1; z_max <= 0 or
 * NaN; tol < 0 or NaN; a null mel / x / z / front / counts / workspace; what wn_iaf_generate_form refuses.  WN_ENOMEM: a
 * workspace below wn_iaf_encode_workspace_bytes, which is 0 for whatever the call would refuse. */
WN_API size_t wn_iaf_encode_workspace_bytes(const wn_handle* h, int form, int B, int F);
WN_API int wn_iaf_encode(wn_handle* h, int form, const float* mel, int B, int F, const float* x, float* z,
                  int n_sweeps, float z_max, float tol, int first, float* mean_tot, float* scale_tot,
                  int32_t* front, int32_t* counts, void* ws, size_t ws_bytes, void* stream);
/* log p(x[t]) = log f(z[t]) - log scale_tot[t] of the student's density at x = z scale_tot + mean_tot: f is Logistic(0,1),
 * log f(z) = -z - 2 softplus(-z), for loss_type logistic and Normal(0,1) for gauss.  The untruncated density: the
 * reference draws u ~ U(1e-5, 1 - 1e-5), which cuts the logistic off at |z| = 11.5; that clip is ignored here.
 * log_prob [B,T] float32 (optional), row_sums [B] float64 (optional): each row summed in double in a fixed order, so
 * repeated calls give the same bits.  Evaluated in double, rounded once.  Refused: a teacher handle, a null z or
 * scale_tot, B < 1 or T < 1. */
WN_API int wn_iaf_latent_log_prob(wn_handle* h, const float* z, const float* scale_tot, int B, int64_t T,
                           float* log_prob, double* row_sums, void* stream);

/* _clip_quant_scale on its own (parallel_wavenet.py:347-359 with
 * utils.cast_quantize / inv_cast_quantize / inv_mu_law, utils.py:108-159):
 * x[n] -> wav[n], idx[n].  Bit-exact integer index. */
WN_API int wn_clip_quant(wn_handle* h, const float* x, int64_t n,
                  float* wav, int32_t* idx, void* stream);

/* ---- log-mel featuriser of the generation drivers (auxilaries/mel_extractor.py:31-44 melspectrogram,
 * :65-90 stft / mel basis / amp_to_db / normalise; called by eval_wavenet.py / eval_parallel_wavenet.py on the
 * host through librosa).  Needs no model handle; errors are reported through wn_last_error(NULL). ---- */

/* Frames of an utterance of n_samples: 1 + n_samples / 200 (centred frames, hop 12.5 ms at 16 kHz). */
WN_API int64_t wn_mel_frames(int64_t n_samples);

/* wav [B][L] float32 (device) -> mel [B][wn_mel_frames(L)][80] float32 (device), values in [0, 1]:
 * reflect-padded centred 2048-point frames, periodic Hann window of 800 samples, |STFT|, Slaney mel basis
 * (80 bands, 125-7600 Hz), 20 log10(max(1e-5, .)), clip((S + 140) / 140, 0, 1).  L must exceed 1024 (the reflect
 * padding, as in numpy.pad). */
WN_API int wn_mel_spectrogram(const float* wav, int B, int64_t L, float* mel, void* stream);

/* ---- the batch of one training step, cut from a device-resident dataset (replaces the queue of
 * auxilaries/reader.py:61-108).  Needs no model handle; errors are reported through wn_last_error(NULL). ---- */

/* pool: every utterance back to back (device, float32); utterance i is pool[utt_off[i] .. utt_off[i] + utt_len[i]).
 * eligible: the indices of the utterances with utt_len >= L (n_eligible of them; all three tables on the device).
 * Row b of stream s takes the words r of Philox4x32-10 under key (seed lo, seed hi) and counter (step lo, step hi, b, s):
 *   u = eligible[(r0 * n_eligible) >> 32],  start = (r1 * (utt_len[u] - L + 1)) >> 32    (64-bit products)
 * -- uniform over the eligible utterances with replacement and over the starts tf.random_crop can return, a function of
 * (seed, step, b, s) alone.  Stream 0 is the batch: wav [B][L] = the crop, mel = its log-mel as wn_mel_spectrogram
 * computes it for the crop (bit for bit; reflect padding at the crop's edges, no load outside the crop).  n_streams = 2
 * adds stream 1, a second unrelated draw of which only the mel is produced (the reference's mel_rand).
 *   wav   [B][L]                                    stream 0 only
 *   mel   [n_streams][B][wn_mel_frames(L)][80]
 *   picks [n_streams][B][2] = (utterance index, start)
 * One launch, asynchronous on `stream`, no workspace, no allocation after the first call on a device, no host
 * synchronisation; every output element has one writer.  WN_EINVAL: a null pointer, B < 1, L <= 1024 (as
 * wn_mel_spectrogram), n_eligible < 1, n_streams not 1 or 2.  The tables are the caller's contract: an `eligible` entry
 * whose utterance is shorter than L, or an utt_off / utt_len outside the pool, is not detected. */
WN_API int wn_train_batch(const float* pool, const int64_t* utt_off, const int64_t* utt_len,
                          const int32_t* eligible, int n_eligible,
                          int B, int64_t L, uint64_t seed, uint64_t step, int n_streams,
                          float* wav, float* mel, int64_t* picks, void* stream);

/* ---- autoregressive path (wavenet.py:379-514, fastgen.py:118-169) ---- */

/* Number of injected random values per sample and per batch element:
 * mol: mol_mix uniforms for the Gumbel-max + 1 uniform for the logistic;
 * gauss: 1 standard normal; ce: 1 uniform in [0,1) (inverse-CDF draw). */
WN_API int wn_ar_n_rand(const wn_handle* h);

/* Bytes of the explicit FIFO state (two queues per causal layer,
 * masked.py:352-355) for batch B. */
WN_API size_t wn_ar_state_bytes(const wn_handle* h, int B);

/* sess.run(init_ops) (fastgen.py:150): zero the queues, step counter := 0. */
WN_API int wn_ar_reset(wn_handle* h, void* state, int B, void* stream);

/* One sess.run([sample, push_ops]) (fastgen.py:158-161):
 *   wav_in   [B]      previous audio sample (float, already de-quantised)
 *   enc_t    [B,deconv_width]  conditioning for this step
 *   rnd      [B,n_rand] injected randoms, or NULL -> Philox(seed, step)
 *   sample   [B]      int32 in [-Q/2,Q/2)
 *   out_params [B,out_width] pre-sampling network output            (optional) */
WN_API int wn_ar_step(wn_handle* h, void* state, int B,
               const float* wav_in, const float* enc_t,
               const float* rnd, uint64_t seed,
               int32_t* sample, float* out_params, void* stream);

/* The whole loop of fastgen.synthesis (fastgen.py:150-168) for Tn steps:
 *   enc   [B,Tn,deconv_width]  (reference layout, e.g. from wn_deconv)
 *   rnd   [Tn,B,n_rand] or NULL -> Philox(seed)
 *   idx   [B,Tn] int32, wav [B,Tn] float (de-quantised feedback signal)
 *   forced_wav [B,Tn] optional teacher forcing: when non-NULL the network input
 *              at step t is forced_wav[:,t-1] instead of its own sample
 *   out_params [B,Tn,out_width] optional */
WN_API int wn_ar_generate(wn_handle* h, const float* enc, int B, int Tn,
                   const float* rnd, uint64_t seed,
                   int32_t* idx, float* wav,
                   const float* forced_wav, float* out_params,
                   void* ws, size_t ws_bytes, void* stream);

/* Fastgen.cond_vars / fastgen.calculate_cond_vars (wavenet/wavenet.py:353-377, wavenet/fastgen.py:91-115): the 1x1
 * conditioning projections of every layer and of the output stage, in bulk over time, biases included.
 * enc [B,Tn,deconv_width] (wn_deconv's output); out: num_layers tensors [B,Tn,gate_width] ('mel_cond_1' ..
 * 'mel_cond_<num_layers>') back to back, then 'mel_cond_out1' [B,Tn,skip_width] -- wn_ar_cond_vars_floats(h,B,Tn) floats. */
WN_API size_t wn_ar_cond_vars_floats(const wn_handle* h, int B, int Tn);
WN_API int wn_ar_cond_vars(wn_handle* h, const float* enc, int B, int Tn, float* out, void* stream);

/* wn_ar_generate replays the step from a hipGraph (16 steps per graph) when the caller's stream can be
 * captured (any stream but the legacy null stream); enable = 0 makes it issue plain launches instead
 * (A/B measurements, graph-vs-launch parity tests).  Default: enabled.  The steps are captured on a private
 * stream of the handle and replayed on the caller's, which is never in capture mode; a capture that fails or is
 * invalidated from outside (a device-wide synchronise of another thread) falls back to plain launches by itself. */
WN_API int wn_ar_set_graph(wn_handle* h, int enable);

/* Full-sequence teacher forward, `Wavenet.feed_forward` (wavenet/wavenet.py:180-291) for a teacher
 * handle: wav [B,T] raw audio in [-1,1] (the input encoding of wavenet.py:412-418 -- mu-law/128 when
 * use_mu_law -- is applied on the device), mel [B,F,n_mel]; out_params [B,T,out_width] are the
 * logits / mixture parameters the reference returns under 'out_params'.  T <= F*frame_shift (the
 * conditioning is centre-cropped to T, wavenet.py:76-85) and T must be a multiple of
 * 2^(num_stages-1) (masked.py:188).  Same result as wn_ar_generate with forced_wav (the reference's
 * incremental == full-sequence identity), T times fewer dependent launches. */
WN_API size_t wn_teacher_workspace_bytes(const wn_handle* h, int B, int F, int64_t T);
WN_API int wn_teacher_forward(wn_handle* h, const float* wav, const float* mel, int B, int F, int64_t T,
                       float* out_params, void* ws, size_t ws_bytes, void* stream);

/* Teacher scoring, the per-sample term of `Wavenet.calculate_loss` (wavenet/wavenet.py:293-316): log-likelihood of the
 * audio wav [B,T] under out_params [B,T,out_width] (what wn_teacher_forward wrote) -- loss_func.mol_log_probs
 * (wavenet/loss_func.py:22-63), gauss_log_prob (:104-119) or the negated cross entropy of ce_loss (:128-133), by the
 * handle's loss_type, on the targets `Wavenet.encode_signal` derives from the raw audio (wavenet.py:157-178: mu-law / 128
 * and the class index when use_mu_law, the audio itself otherwise).  log_prob [B,T]; the reference's scalar loss is
 * minus its mean.  Asynchronous on `stream`; no workspace.
 * Accuracy contract (what "parity" means here): the values are the float64-accurate ones of the reference's FORMULAS.  The
 * mixture-of-logistics bin mass is formed as sigma(a) sigma(-b) (1 - e^-(a-b)) with a - b computed directly; the reference's
 * float32 graph evaluates sigmoid(plus) - sigmoid(min), which keeps about two digits of a mass of 1/65 536 -- a loss printed
 * by a float32 TensorFlow run of the reference can therefore differ from this one in its third digit, by the reference's own
 * cancellation, not by this path's error (tests hold 2e-5 against the float64 evaluation of the reference's code).  The
 * mu-law class of a sample closer than ~1e-5 of a bin to a bin edge is decided by the rounding of a float32 log in any
 * implementation; 1e-3 of a bin away from every edge the class is exact (tests/test_gpu_teacher.py). */
WN_API int wn_teacher_log_prob(wn_handle* h, const float* out_params, const float* wav, int B, int64_t T, float* log_prob,
                        void* stream);

/* Gradient of wn_teacher_log_prob: with g = d_log_prob[b,t] ([B,T], the derivative of the caller's loss with
 * respect to log_prob -- -1 / (B T) everywhere for Wavenet.calculate_loss's 'loss'), d_out_params [B,T,out_width] and, when
 * d_wav is not NULL, d_wav [B,T] through the TARGET (the path through the network input is wn_teacher_backward_input's).
 *   mol    r_i = exp(v_i + logsoftmax(lg)_i - log_prob) with v_i the component's log-probability;
 *          d lg_i = g (r_i - softmax(lg)_i); d mean_i = -g r_i dx_i; d log_s_i = -g r_i dinv_i inv_s_i where the raw
 *          log-scale is >= -7, 0 below; d wav = g sum_i r_i dx_i  (dx_i = d v_i / d x, dinv_i = d v_i / d inv_s_i)
 *   gauss  z = (x - m) e^-ls: d m = g z e^-ls; d p = g (z^2 - 1) where p >= -7, 0 below; d wav = -g z e^-ls
 *   ce     d logit_k = g (onehot_k - softmax_k), the label formed as in the forward
 * on the forward's targets, class count, thresholds and form of the bin mass, with the tie conventions listed under the
 * distillation gradients below (tf.maximum at -7 and at the 1e-12 floor, tf.where at the edge bins).
 * d_wav is ZERO for every mu-law teacher and every ce teacher: Wavenet.encode_signal quantises the audio before the target
 * is used, the target is piecewise constant in wav and TensorFlow propagates nothing through it.
 * A work call like the forward: asynchronous on `stream`, no workspace, no allocation, no host synchronisation, safe from
 * several threads on one handle; every output element has one writer (no atomics), so a repeated call is bit-identical.
 * Overwrites its outputs.  A 256-class row is read once (it stays in registers), a 65 536-class row twice (running max /
 * sum, then the softmax) and written once.  WN_EINVAL (message in wn_last_error): a null or student handle, B or T < 1, a
 * null out_params / wav / d_log_prob / d_out_params, and the ce width mismatch the forward refuses. */
WN_API int wn_teacher_log_prob_grad(wn_handle* h, const float* out_params, const float* wav, int B, int64_t T,
                                    const float* d_log_prob, float* d_out_params, float* d_wav, void* stream);

/* ---- distillation losses (ParallelWavenet.kl_loss_logistic / kl_loss_gauss / power_loss, wavenet/parallel_wavenet.py:361-479)
 * scored under a TEACHER handle on the out_params wn_teacher_forward wrote for the student's unclipped audio x.
 * Each call refuses with WN_EINVAL (message in wn_last_error): a student handle; a ce teacher in the mol call; a non-gauss
 * teacher in the gauss call; any mu-law teacher (the reference would score mu-law encoded audio unencoded there, CLIP = False);
 * num_samples S < 1; an out_width that is not the handle's.  Asynchronous on `stream`, no allocation, no synchronisation;
 * every sum is reduced in a fixed order, so a repeated call is bit-identical.  `sums` are two float64 values on the device. ---- */

/* Workspace of wn_distill_mol_xent and wn_distill_gauss_kl for B utterances of T samples. */
WN_API size_t wn_distill_workspace_bytes(const wn_handle* h, int B, int64_t T);

/* Monte-Carlo cross entropy of kl_loss_logistic (:361-402): for every row (b, t) and draw s, x = rl[b,s,t] * scale_tot[b,t]
 * + mean_tot[b,t] is scored by loss_func.mol_log_probs (wavenet/loss_func.py:22-63, Q = 65536, x not quantised) under
 * out_params[b,t,:] [B,T,out_width = 3 mol_mix]; h_bl[b,t] = -mean_s log p ([B,T], the reference's H_Ps_Pt_bl);
 * sums[0] = sum of h_bl, sums[1] = sum of log scale_tot -- H_Ps_Pt = sums[0] / (B T), H_Ps = sums[1] / (B T) + 2.
 *   noise      [B,S,T] injected logistic draws (row b*S + s of the reference's [B*S,T] draw, utils.tf_repeat), or NULL:
 *              drawn on the device, Philox4x32-10 keyed by (seed; b, s, t), log u - log(1-u), u ~ U(1e-5, 1-1e-5)
 *   noise_out  [B,S,T] the draws used (optional)
 * No [B,S,T,.] intermediate exists: each teacher row is read once and its S draws are evaluated in registers. */
WN_API int wn_distill_mol_xent(wn_handle* h, const float* out_params, int out_width, const float* mean_tot,
                               const float* scale_tot, int B, int64_t T, int S, const float* noise, uint64_t seed,
                               float* h_bl, float* noise_out, double* sums, void* ws, size_t ws_bytes, void* stream);

/* Closed-form Gaussian KL of kl_loss_gauss (:404-429) on out_params [B,T,2] (mean, log scale; loss_func.py:66-75):
 * kl_bl[b,t] [B,T]; sums[0] = sum of kl_bl, sums[1] = sum of (log s_p - log s_q)^2 -- kl_loss = (sums[0] + 4 sums[1]) / (B T). */
WN_API int wn_distill_gauss_kl(wn_handle* h, const float* out_params, int out_width, const float* mean_tot,
                               const float* scale_tot, int B, int64_t T, float* kl_bl, double* sums, void* ws,
                               size_t ws_bytes, void* stream);

/* power_loss (:459-479) with the reference's module constants (|STFT|, squared difference, USE_PRIORITY_FREQ): pred and orig
 * rows of L samples (row strides pred_stride / orig_stride floats: the centre trim of the longer signal, :431-436, is a
 * pointer offset), tf.contrib.signal.stft(frame_length 800, frame_step 200, fft_length 2048, pad_end=True) -- ceil(L/200)
 * frames of 1025 bins, periodic Hann window, not centred.  out2[0] = sum over (b, frame, bin) of (|P| - |O|)^2, out2[1] the
 * same over the bins below 384 (mel_extractor.PRIORITY_FREQ): power_loss = 0.5 out2[0] / (B NF 1025) + 0.5 out2[1] / (B NF 384).
 * Needs no handle; errors through wn_last_error(NULL). */
WN_API size_t wn_power_loss_workspace_bytes(int B, int64_t L);
WN_API int wn_power_loss(const float* pred, int64_t pred_stride, const float* orig, int64_t orig_stride, int B, int64_t L,
                         double* out2, void* ws, size_t ws_bytes, void* stream);

/* ---- gradients of the distillation losses with respect to the student's x, mean_tot and scale_tot.
 * The teacher is frozen: only its input VJP runs, no weight gradient.  Work calls like the losses above: asynchronous on
 * `stream`, no allocation, no host synchronisation, safe from several threads on one handle (own workspaces and streams);
 * no atomics, so a repeated call is bit-identical.  `fac` is two float64 values ON THE DEVICE: the derivative of the
 * caller's loss with respect to the two sums the matching forward call returns (sums / out2), so a backward pass reads
 * nothing back to the host.  They refuse what the forward calls refuse (student handle, ce teacher, mu-law teacher,
 * mismatched pairing, num_samples < 1, wrong out_width) with WN_EINVAL.
 * Tie conventions are TensorFlow's, i.e. the gradient TF's autodiff gives for the reference's graph:
 *   tf.maximum(log_s, -7)   passes the gradient where log_s >= -7, none below;
 *   tf.maximum(mass, 1e-12) passes the gradient where mass >= 1e-12, none below the floor;
 *   tf.where (edge bins)    the selected branch only;
 *   relu                    where the pre-activation is > 0;
 *   |z| of the STFT         gradient 0 at z = 0.
 * The MoL bin mass is differentiated in the form the forward evaluates, sigma(a) sigma(-b) (1 - e^-(a-b)) with
 * a - b = 2 inv_s / Q (wn_mol.h), not as a float32 difference of sigmoids: the same function, without the cancellation. ---- */

/* Tape of the teacher forward for B utterances of T samples: a 256-byte header (handle identity, B, T, layer count), the
 * pre-ReLU skip sum and out1 rows, and sigma / tanh of every gate -- 4 (2 skip_width + num_layers gate_width) bytes per
 * sample with T rounded up to 256 (wavenet_mol.json: 30 * 512 * 4 B of gates per sample, 4.7 GB at B = 1, T = 76 800). */
WN_API size_t wn_teacher_tape_bytes(const wn_handle* h, int B, int64_t T);
/* wn_teacher_forward (same arguments, same workspace, bit-identical out_params) that also writes the tape. */
WN_API int wn_teacher_forward_tape(wn_handle* h, const float* wav, const float* mel, int B, int F, int64_t T,
                                   float* out_params, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes, void* stream);
/* Input VJP: d_wav [B,T] = (d out_params / d wav)^T d_out_params [B,T,out_width], on a tape this handle's
 * wn_teacher_forward_tape wrote for the same B and T (any other tape is refused with WN_EINVAL).  The transposed GEMMs run
 * on the forward's split-fp16 MFMA kernel; d_out_params enter scaled by the power of two that brings their largest
 * magnitude to [1, 2), found on the device.  Needs width, skip_width and gate_width / 2 multiples of 64. */
WN_API size_t wn_teacher_backward_workspace_bytes(const wn_handle* h, int B, int64_t T);
WN_API int wn_teacher_backward_input(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_out_params, int B,
                                     int64_t T, float* d_wav, void* ws, size_t ws_bytes, void* stream);

/* ---- weight gradients of the teacher: the reverse pass of wn_teacher_backward_input, run once, that also
 * returns the gradient of every variable of the residual stack and output head, and the cotangent of the conditioning.
 * MoL and Gauss teachers without mu-law, as the input VJP; mu-law and ce teachers stay out of scope (the ce head fails
 * out_width <= 64), and so do weight-norm configurations and shapes whose width, skip_width or gate_width / 2 is no
 * multiple of 64: all refused with WN_EINVAL.  Work calls: asynchronous on `stream`, no allocation, no host
 * synchronisation, no atomics -- every output element has one writer and a repeated call is bit-identical.
 *
 * The gradients live in ONE flat float32 buffer of wn_teacher_grad_floats(h) floats.  wn_teacher_grad_count /
 * wn_teacher_grad_info give, in a fixed order (conv_start, skip_start, per layer dilated_conv_i, mel_cond_i, res_i, skip_i,
 * then out1, mel_cond_out1, out2; W before biases), the TensorFlow variable name (NUL-terminated into name[name_cap]), the
 * float offset and the TF shape (shape4[0 .. ndim-1]; [1, K, in, out] kernels, [out] biases) of gradient i. ---- */
WN_API int wn_teacher_grad_count(const wn_handle* h);
WN_API int wn_teacher_grad_info(const wn_handle* h, int i, char* name, size_t name_cap, int64_t* offset, int64_t* shape4,
                                int* ndim);
WN_API size_t wn_teacher_grad_floats(const wn_handle* h);
/* Training tape: the tape of wn_teacher_forward_tape (the same bytes at the same offsets) followed by the input l_i of every
 * residual layer (split-fp16 rows with their zero left pad), the conditioning as deconvolved for F mel frames, and the
 * scaled audio row.  wn_teacher_backward_input accepts it in place of a plain tape.  This and the workspace query below
 * return 0 for a handle the work calls refuse. */
WN_API size_t wn_teacher_train_tape_bytes(const wn_handle* h, int B, int F, int64_t T);
/* wn_teacher_forward (same arguments, same workspace, bit-identical out_params) that also writes the training tape. */
WN_API int wn_teacher_forward_train_tape(wn_handle* h, const float* wav, const float* mel, int B, int F, int64_t T,
                                         float* out_params, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                         void* stream);
WN_API size_t wn_teacher_backward_weights_workspace_bytes(const wn_handle* h, int B, int F, int64_t T);
/* d_out_params [B,T,out_width] -> grads (every element overwritten; grads_floats >= wn_teacher_grad_floats), and when not
 * NULL d_encoding [B, F frame_shift, deconv_width] (zero outside the centre crop of T columns; needs deconv_width % 64 == 0)
 * and d_wav [B,T] -- the bits wn_teacher_backward_input returns.  The tape must be a TRAINING tape this handle wrote for
 * the same B, F and T; a plain tape is refused.  The time reductions walk valid columns only: nothing the tape or the
 * workspace holds at columns [T, round_up(T, 256)) reaches a result. */
WN_API int wn_teacher_backward_weights(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_out_params, int B,
                                       int F, int64_t T, float* grads, size_t grads_floats, float* d_encoding, float* d_wav,
                                       void* ws, size_t ws_bytes, void* stream);

/* ---- dropout of the teacher's training pass: tf.layers.dropout(training=True) of wavenet.py:204-239, 276-278.
 * wn_config does not carry the dropout keys: mode, seed and rate come per call.
 *   WN_DROPOUT_INPUTS  site 0 = conv_dropout on l_0 (width channels), site 1 = skip_dropout on s = skip_start(l_0), both applied
 *                      AFTER skip_start has read the undropped l_0;
 *   WN_DROPOUT_ALL     site 0 = conv_dropout on l_0 before skip_start reads it, site i = res_dropout_i on the output of
 *                      residual layer i = 1 .. num_layers - 1 (the last layer's output is read by nothing).
 * The mask is a stateless counter hash: element (b, c, t) of `site` is kept where word (t & 3) of Philox4x32-10 with
 * key = seed and counter = (t >> 2, c, site, b) is >= thr = min(2^32 - 1, floor(rate 2^32 + 0.5)) -- a function of these
 * values alone, whatever the launch geometry.  A kept element is fp32(v / fp32(1 - rate)), a dropped one is 0.
 * rate = 0 keeps everything and gives the bits of the calls without dropout. */
#define WN_DROPOUT_INPUTS 1
#define WN_DROPOUT_ALL    2
/* Bytes of a dropout training tape: the training tape (the same bytes at the same offsets), and for WN_DROPOUT_INPUTS one more
 * l row behind it, the undropped l_0 that skip_start/W's gradient multiplies.  0 for a handle the work call refuses or an
 * unknown mode. */
WN_API size_t wn_teacher_train_tape_dropout_bytes(const wn_handle* h, int B, int F, int64_t T, int mode);
/* wn_teacher_forward_train_tape (same arguments, same workspace) with dropout: out_params are those of the dropped forward.
 * The tape remembers mode, seed and rate: wn_teacher_backward_weights and wn_teacher_backward_input accept it and apply the
 * same masks to the cotangents, with their own signatures and workspace sizes.  Refuses what wn_teacher_forward_train_tape
 * refuses, a rate outside [0, 1) and an unknown mode (WN_EINVAL). */
WN_API int wn_teacher_forward_train_tape_dropout(wn_handle* h, const float* wav, const float* mel, int B, int F, int64_t T,
                                                 float* out_params, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                                 void* stream, int mode, uint64_t seed, double rate);
/* The keep bits themselves, for tests: keep [B][T][C] bytes (1 = kept) of `site`, written by a kernel that only calls the
 * hash the passes above call.  No handle. */
WN_API int wn_teacher_dropout_keep(uint64_t seed, int site, int B, int C, int64_t T, double rate, unsigned char* keep,
                                   void* stream);

/* ---- weight gradients of the ParallelWavenet student: the training forward of the IAF flows onto a tape and
 * one reverse pass over it, on the GEMM kernels of the teacher's training passes.  Student handles with width % 64 == 0 and
 * deconv_width % 64 == 0, without weight norm and without mu-law; any num_iaf_layers and num_stages; shared, teacher or
 * private deconv stacks.  Everything else is refused with WN_EINVAL and the size queries return 0 for it.  T and F obey the
 * rules of wn_iaf_generate: T is a multiple of 2^(num_stages - 1), T <= F frame_shift, and the conditioning is centre-cropped
 * to T columns.  Work calls as above: asynchronous on `stream`, no allocation, no host synchronisation, no atomics -- one
 * writer per output element, a repeated call is bit-identical.
 *
 * The gradients live in ONE flat float32 buffer of wn_iaf_grad_floats(h) floats, laid out like wn_teacher_grad_info's: per
 * flow k = 1 .. in order "iaf_k/start_conv", per layer "iaf_k/dilated_conv_i", "iaf_k/mel_cond_i", "iaf_k/res_i", then
 * "iaf_k/out1", "iaf_k/mel_cond_out1", "iaf_k/out2_mean", "iaf_k/out2_scale"; "/W" in the TF shape before "/biases". ---- */
WN_API int wn_iaf_grad_count(const wn_handle* h);
WN_API int wn_iaf_grad_info(const wn_handle* h, int i, char* name, size_t name_cap, int64_t* offset, int64_t* shape4, int* ndim);
WN_API size_t wn_iaf_grad_floats(const wn_handle* h);
WN_API size_t wn_iaf_train_tape_bytes(const wn_handle* h, int B, int F, int64_t T);
WN_API size_t wn_iaf_train_workspace_bytes(const wn_handle* h, int B, int F, int64_t T);
/* ParallelWavenet.feed_forward on the caller's draw noise [B,T]: mean_tot, scale_tot = min(prod_k scale_k, e^7) and
 * x = noise scale_tot + mean_tot, each [B,T], and the tape wn_iaf_backward_weights reads (identified by its address: a copy
 * is refused). */
WN_API int wn_iaf_forward_train_tape(wn_handle* h, const float* noise, const float* mel, int B, int F, int64_t T, float* x,
                                     float* mean_tot, float* scale_tot, void* tape, size_t tape_bytes, void* ws,
                                     size_t ws_bytes, void* stream);
WN_API size_t wn_iaf_backward_weights_workspace_bytes(const wn_handle* h, int B, int F, int64_t T);
/* d_x, d_mean_tot, d_scale_tot [B,T]: the cotangents of the three RETURNED tensors as independent outputs; the call adds x's
 * dependence on the other two (d mean_tot += d_x; d scale_tot += d_x noise where the e^7 clamp is not active).  grads: every
 * element overwritten (grads_floats >= wn_iaf_grad_floats).  d_encoding: NULL, or float32 [n_stacks, B, F frame_shift,
 * deconv_width], zero outside the centre crop; n_stacks is 1 for a shared or teacher-owned deconv stack (every flow
 * accumulates into it) and the number of flows for private stacks.  Ties: a clamp passes the gradient at the tie and none
 * beyond it, a ReLU at exactly 0 passes none.  The tape must be one this handle wrote for the same B, F and T. */
WN_API int wn_iaf_backward_weights(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_x,
                                   const float* d_mean_tot, const float* d_scale_tot, int B, int F, int64_t T, float* grads,
                                   size_t grads_floats, float* d_encoding, void* ws, size_t ws_bytes, void* stream);
/* The same reverse pass over the same tape without the weight products: the gradient of the student's inputs.
 * d_noise [B,T], every element overwritten: the total derivative of sum(x d_x + mean_tot d_mean_tot + scale_tot d_scale_tot)
 * with the noise as a leaf, of the function wn_iaf_forward_train_tape evaluates -- the chain through every flow down to the
 * first flow's start conv, plus d_x scale_tot for x = noise scale_tot + mean_tot.  d_encoding as above, and bit-equal to what
 * wn_iaf_backward_weights returns for the same tape and cotangents.  Same checks, ties and refusals; a smaller workspace. */
WN_API size_t wn_iaf_backward_input_workspace_bytes(const wn_handle* h, int B, int F, int64_t T);
WN_API int wn_iaf_backward_input(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_x, const float* d_mean_tot,
                                 const float* d_scale_tot, int B, int F, int64_t T, float* d_noise, float* d_encoding, void* ws,
                                 size_t ws_bytes, void* stream);

/* ---- the gradient of the student's log-likelihood.  log p(x) = log f(z) - log scale_tot at z = encode(x).
 * wn_iaf_latent_log_prob_grad is wn_iaf_latent_log_prob's counterpart: for a cotangent d_log_prob [B,T] of log p (NULL: the
 * constant -1 / (B T), the cotangent of -mean log p)
 *   g_z = d_log_prob (log f)'(z)      (log f)' = -tanh(z / 2) for loss_type logistic, -z for gauss
 *   d_scale_tot = -d_log_prob / scale_tot
 * both [B,T] float32, evaluated in double and rounded once; scale_tot is taken as given, as wn_iaf_latent_log_prob takes it.
 * Refused: a teacher handle, a null z / scale_tot / g_z / d_scale_tot, B < 1 or T < 1. */
WN_API int wn_iaf_latent_log_prob_grad(wn_handle* h, const float* z, const float* scale_tot, int B, int64_t T,
                                       const float* d_log_prob, float* g_z, float* d_scale_tot, void* stream);
/* The adjoint of the inverse.  On a tape wn_iaf_forward_train_tape wrote at noise = z, with A = d x / d noise (lower
 * triangular, diagonal scale_tot), the call solves A^T lam = g_z + (d mean_tot / d noise)^T d_mean_tot + (d scale_tot /
 * d noise)^T d_scale_tot by n_sweeps Jacobi sweeps, enqueued without a host synchronisation:
 *   lam <- lam + (g_z + r) / min(scale_tot, e^7),   r = d_noise of wn_iaf_backward_input(tape, -lam, d_mean_tot, d_scale_tot)
 * A^T is upper triangular: after k sweeps the last k samples of a row are exact, after T sweeps the row.  With the outputs of
 * wn_iaf_latent_log_prob_grad, lam is the gradient with respect to x, and wn_iaf_backward_weights(tape, -lam, 0, d_scale_tot)
 * gives those of the weights and the encoding.
 *   lam         [B,T]: the starting iterate on entry, the last sweep's on return
 *   d_mean_tot  [B,T] or NULL (zero)
 *   tol         a row has converged when its last sweep had max |lam' - lam| <= tol max |lam'|
 *   resid       float [B][2]: max |lam' - lam| and max |lam'| of the row in the last sweep
 *   counts      int32 [4]: [0] values of the last sweep that were not finite and were replaced by 0; [1] rows above tol in
 *               the last sweep; [2] the first sweep of this call, counted from 1, after which every row had converged and
 *               nothing was replaced, 0 if none -- the call's later sweeps then change nothing: lam and resid are that
 *               sweep's; [3] 0
 * No atomics: a repeated call gives the same bits.  Refused as wn_iaf_backward_input refuses (handle, shape, tape), and:
 * n_sweeps < 1, tol < 0 or NaN, a null tape / g_z / d_scale_tot / lam / resid / counts / workspace (WN_EINVAL); a workspace
 * below wn_iaf_adjoint_workspace_bytes (WN_ENOMEM), which is 0 for a handle or a shape the call refuses. */
WN_API size_t wn_iaf_adjoint_workspace_bytes(const wn_handle* h, int B, int F, int64_t T);
WN_API int wn_iaf_adjoint(wn_handle* h, const void* tape, size_t tape_bytes, const float* g_z, const float* d_mean_tot,
                          const float* d_scale_tot, int B, int F, int64_t T, float* lam, int n_sweeps, float tol, float* resid,
                          int32_t* counts, void* ws, size_t ws_bytes, void* stream);

/* ---- reverse pass of the upsampler: the gradients of trans_conv_j/kernel and trans_conv_j/bias of the deconv
 * stack `scope` ("" for a teacher; "iaf_share", "iaf_1" ... for a student, as in wn_deconv) from mel [B,F,n_mel] and a
 * cotangent d_enc [B, F frame_shift, deconv_width] of wn_deconv's output, e.g. d_encoding of wn_teacher_backward_weights.
 * A separate call: it reruns the stack's forward into its own workspace and neither reads nor changes a teacher tape; the
 * wn_teacher_grad_* table is not affected.  Split-fp16 arithmetic whatever the handle's precision; the cotangent enters
 * scaled by the power of two that brings its largest magnitude to [1, 2), so a cotangent scaled by 2^k gives the same
 * gradients scaled bit for bit.  No atomics, one writer per element: a repeated call is bit-identical.  A work call:
 * asynchronous on `stream`, no allocation, no host synchronisation.
 * Refused with WN_EINVAL (message in wn_last_error): use_resize_conv, use_weight_norm, a deconv_width that is no multiple of
 * 64, a layer without split-fp16 pack, a stride above 30, an unknown scope, grads_floats or ws_bytes too small.  The count
 * and size queries return 0 for what the work call refuses.  A handle that is not finalized: WN_ESTATE, as wn_deconv.
 * Cost for every handle, trained or not: wn_finalize packs a transposed split-fp16 copy of the kernel of every deconv
 * layer but the first of a stack (K Cin Cout 4 bytes: 21 MB for the shipped 80 x 256 x 256 layer, once per stack) at the end
 * of the handle's device blob; no existing offset moves.
 * Table, per layer j = 1 .. in order: "<scope/>trans_conv_j/kernel" [1, K, Cout, Cin], then "<scope/>trans_conv_j/bias"
 * [Cout]; name / offset / shape as in wn_teacher_grad_info. ---- */
WN_API int wn_deconv_grad_count(const wn_handle* h, const char* scope);
WN_API int wn_deconv_grad_info(const wn_handle* h, const char* scope, int i, char* name, size_t name_cap, int64_t* offset,
                               int64_t* shape4, int* ndim);
WN_API size_t wn_deconv_grad_floats(const wn_handle* h, const char* scope);
WN_API size_t wn_deconv_backward_workspace_bytes(const wn_handle* h, const char* scope, int B, int F);
/* grads: every element of the first wn_deconv_grad_floats floats is overwritten.  d mel is not computed here: see
 * wn_deconv_backward_input. */
WN_API int wn_deconv_backward(wn_handle* h, const char* scope, const float* mel, const float* d_enc, int B, int F, float* grads,
                              size_t grads_floats, void* ws, size_t ws_bytes, void* stream);
/* d mel of the stack: d_mel [B,F,n_mel], every element overwritten, from the same mel and d_enc.  The contract
 * of wn_deconv_backward: the forward is rerun in split fp16 into the call's own workspace, each layer's cotangent enters scaled
 * by a power of two (a cotangent scaled by 2^k gives d_mel scaled bit for bit), no atomics, one writer per element, the same
 * refusals; the size query returns 0 for what the work call refuses.  Only the data-gradient chain runs -- no weight or bias
 * gradient.  Cost for every handle: wn_finalize packs one more transposed split-fp16 copy, the first layer's kernel with its
 * input channels padded to a multiple of 64 (5.2 MB for the shipped 40 x 80 x 256 layer), behind every other pack. */
WN_API size_t wn_deconv_backward_input_workspace_bytes(const wn_handle* h, const char* scope, int B, int F);
WN_API int wn_deconv_backward_input(wn_handle* h, const char* scope, const float* mel, const float* d_enc, int B, int F,
                                    float* d_mel, void* ws, size_t ws_bytes, void* stream);

/* ---- Teacher training step on the device ----
 *
 * wn_teacher_set_weights rewrites the packed weights of a FINALIZED teacher handle in place from fp32 masters that live on
 * the device.  `params` is a flat buffer in the layout of the gradient table (offsets and TF shapes of wn_teacher_grad_info,
 * wn_teacher_grad_floats floats); `up_params` is the upsampler's, in the layout of wn_deconv_grad_info with scope "", or NULL:
 * the upsampler's packs then stay as they are.  After the call every byte of the handle's device blob that depends on those
 * variables equals what wn_finalize of a fresh handle would have uploaded for the same values: the row-major matrices, summed
 * and composite biases and A-fragment copies of the autoregressive step, every split-fp16 GEMM pack of the full-sequence
 * forward and its transposes, the upsampler's fp32 fragments, bias, split-fp16 pack, phase-group pack and the transposed
 * planes of its reverse pass.  No device pointer of the handle changes and nothing is allocated.
 *
 * No weight and no packed word crosses to the host.  The scale of every split pack needs the largest magnitude of its
 * source: those maxima are reduced on the device into `ws` and READ BACK (a few hundred floats), so the call SYNCHRONISES
 * `stream` once, midway; the kernels behind that point are enqueued and the call returns without waiting for them, so
 * `params` and `up_params` must stay unchanged until `stream` has passed the call (later work on `stream` is ordered).
 *
 * The call takes the handle exclusively, like the switches ("Concurrency"): WN_ESTATE while a work call of another thread is
 * inside the library.  Work enqueued earlier on OTHER streams that reads the handle's weights must have finished: that is
 * the caller's job (work on `stream` itself is ordered).  The handle's tape serial changes: a tape or training tape written
 * before the call is refused afterwards by wn_teacher_backward_input and wn_teacher_backward_weights.
 * If the call fails with WN_EIO after it has begun to launch, the handle's weights are undefined (partly old, partly new)
 * until a later call succeeds; the tape serial has changed by then, so no older tape is accepted.
 * WN_EINVAL: a student handle; a handle the weight-gradient calls refuse (mu-law, ce, weight norm); use_resize_conv with a
 * non-NULL up_params; float counts that are not the tables'; a workspace below wn_teacher_set_weights_workspace_bytes (0 for
 * a handle the call refuses).  WN_ESTATE: a handle that is not finalized. */
WN_API size_t wn_teacher_set_weights_workspace_bytes(const wn_handle* h);
WN_API int wn_teacher_set_weights(wn_handle* h, const float* params, size_t params_floats, const float* up_params,
                                  size_t up_floats, void* ws, size_t ws_bytes, void* stream);

/* ---- Student training step on the device ----
 *
 * wn_iaf_set_weights is wn_teacher_set_weights' counterpart for a FINALIZED student handle.  `params` is a flat device buffer
 * in the layout of wn_iaf_grad_info (wn_iaf_grad_floats floats).  `up_params` is a HOST array of n_up device pointers, one
 * per deconv stack in the order of d_encoding's leading axis (the one stack "iaf_share", or "iaf_k" per flow), each in the
 * layout of wn_deconv_grad_info(h, scope) with up_floats[s] floats; n_up == 0 or a NULL entry: that stack keeps its packs.
 * After the call every word of the device blob that a kernel reads, and every host-side value passed as a kernel argument,
 * equals what wn_finalize of a fresh handle loaded with the same values would have produced: the plain tensors of a generic
 * student (and its two head biases, which are host floats), or the fp32 fragments and the split-fp16 packs of the three
 * launch forms; the GEMM packs of the training calls with their transposes; for every stack handed in, the packs
 * wn_teacher_set_weights rewrites for a teacher's.  Layer ids, row-block tables, launch plans, zero pad rows and the zero
 * biases of transposed packs do not depend on the variables and are left alone.  No pointer changes, nothing is allocated.
 *
 * The call is table-driven: one launch per KIND of pack over a descriptor table built on the host and uploaded into `ws`, so
 * its launch count depends on the number of deconv stacks handed in, not on flows or layers.  The maxima behind the scales
 * (and a generic student's head biases) are READ BACK: the call SYNCHRONISES `stream` once, midway, and returns with the
 * rest enqueued; `params`, the stacks' buffers and `ws` must stay unchanged until `stream` has passed the call.
 *
 * Exclusive like the switches ("Concurrency"): WN_ESTATE while a work call of another thread is inside the library; work
 * enqueued earlier on other streams that reads the handle's weights must have finished.  The handle's tape serial changes
 * before the first launch: a tape of wn_iaf_forward_train_tape written before the call is refused afterwards, also after a
 * failure midway (the weights are then undefined until a later call succeeds).
 * WN_EINVAL, by name: a teacher handle; a handle the student's training calls refuse (mu-law, weight norm, width or
 * deconv_width no multiple of 64); n_up neither 0 nor the number of stacks; a float count that is not the table's;
 * use_resize_conv with a non-NULL entry; a workspace below wn_iaf_set_weights_workspace_bytes (0 for a handle the call
 * refuses).  WN_ESTATE: a handle that is not finalized. */
WN_API size_t wn_iaf_set_weights_workspace_bytes(const wn_handle* h);
WN_API int wn_iaf_set_weights(wn_handle* h, const float* params, size_t params_floats, const float* const* up_params,
                              const size_t* up_floats, int n_up, void* ws, size_t ws_bytes, void* stream);

/* Sum of squares of n device floats in double: a fixed-order two-stage reduction without atomics (a repeated call gives the
 * same bits).  acc[0] (one device double) is written, or added to when `accumulate` is non-zero, so that the buffers of the
 * residual stack and of the upsampler chain into one global norm.  Needs no handle; errors through wn_last_error(NULL).
 * Asynchronous on `stream`. */
WN_API size_t wn_grad_sumsq_workspace_bytes(size_t n);
WN_API int wn_grad_sumsq(const float* g, size_t n, double* acc, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* Combine the gradients of S shards of one training step: with r_j = rows + j * row_stride,
 *   out[i] = (((r_0[i] + r_1[i]) + r_2[i]) + ... + r_{S-1}[i]) * (1.0f / S)   for i < n,
 * in float32, strictly left to right with one rounding per add and one for the product, so the result depends on the
 * rows and their order alone -- not on how the shards were spread over devices.  S in [1, 64] (S = 1: a copy times 1);
 * row_stride >= n floats; `out` may be row 0 and must not overlap any other row.  One writer per element, no atomics: a
 * repeated call gives the same bits.  16-byte accesses with a scalar tail (all scalar when rows, out or row_stride * 4 is
 * off the 16-byte grid); any n >= 1.  Needs no handle; errors through wn_last_error(NULL).  Asynchronous on `stream`. */
WN_API int wn_grad_combine(const float* rows, size_t n, size_t row_stride, int S, float* out, void* stream);

/* One step of TensorFlow's Adam on n device floats, with the shadow of tf.train.ExponentialMovingAverage:
 *   m <- beta1 m + (1 - beta1) g',  v <- beta2 v + (1 - beta2) g'^2,  p <- p - lr_t m / (sqrt(v) + eps),
 *   ema <- ema - (1 - ema_decay_t) (ema - p)   on the updated p (ema may be NULL).
 * lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) is formed by the caller.  With sumsq non-NULL (one device double, the squared
 * global norm of wn_grad_sumsq), g' = g clip_norm / max(sqrt(sumsq[0]), clip_norm) -- tf.clip_by_global_norm, read on the
 * device -- otherwise g' = g.  Each element is formed in double from the fp32 state and every stored value is rounded once.
 * 16-byte accesses with a scalar tail (all scalar when a pointer is off the 16-byte grid); any n >= 1.  Needs no handle;
 * asynchronous on `stream`. */
WN_API int wn_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr_t, float beta1,
                            float beta2, float eps, float ema_decay_t, const double* sumsq, float clip_norm, void* stream);

/* Gradient of L = fac[0] sums[0] + fac[1] sums[1] of wn_distill_mol_xent (same draws: `noise`, or Philox under `seed`):
 * d_out_params [B,T,3 mol_mix], d_mean_tot and d_scale_tot [B,T] (through x = rl scale_tot + mean_tot, and 1 / scale_tot of
 * the log scale_tot sum).  Overwrites its outputs; no workspace. */
WN_API int wn_distill_mol_xent_grad(wn_handle* h, const float* out_params, int out_width, const float* mean_tot,
                                    const float* scale_tot, int B, int64_t T, int S, const float* noise, uint64_t seed,
                                    const double* fac, float* d_out_params, float* d_mean_tot, float* d_scale_tot,
                                    void* stream);
/* Gradient of L = fac[0] sums[0] + fac[1] sums[1] of wn_distill_gauss_kl: d_out_params [B,T,2], d_mean_tot, d_scale_tot. */
WN_API int wn_distill_gauss_kl_grad(wn_handle* h, const float* out_params, int out_width, const float* mean_tot,
                                    const float* scale_tot, int B, int64_t T, const double* fac, float* d_out_params,
                                    float* d_mean_tot, float* d_scale_tot, void* stream);
/* Gradient of L = fac[0] out2[0] + fac[1] out2[1] of wn_power_loss with respect to pred: d_pred rows of L samples (row
 * stride d_pred_stride).  Per frame the bins' 2 (|P| - |O|) P / |P| go back through the DFT and the window; the frames are
 * overlap-added in a fixed order.  Needs no handle; errors through wn_last_error(NULL). */
WN_API size_t wn_power_loss_grad_workspace_bytes(int B, int64_t L);
WN_API int wn_power_loss_grad(const float* pred, int64_t pred_stride, const float* orig, int64_t orig_stride, int B,
                              int64_t L, const double* fac, float* d_pred, int64_t d_pred_stride, void* ws, size_t ws_bytes,
                              void* stream);

/* 1 when wn_iaf_generate(B, F) evaluates the per-layer conditioning 1x1s in one hoisted GEMM per
 * deconv stack (the default of the split-fp16 path: the layer kernels then stream 768 B/sample
 * instead of 1536 and the small-dilation layers run two per launch; since round 6 also the default of the fp32 form:
 * one fp32 GEMM per deconv stack, the layer kernels on the dilated conv alone), 0 for cond_mode 1 (fused), for fp32
 * calls whose length is not a multiple of 128 samples and for calls whose projected term would not fit (cond_mode 0). */
WN_API int wn_iaf_cond_hoisted(const wn_handle* h, int B, int F);

/* 1 when wn_iaf_generate(B, F) runs the residual layers in layer groups (up to five layers per launch with the residual
 * stream in LDS: one natural and one decimated group per ten-layer dilation cycle) -- the default of the hoisted form
 * whenever the flows split into alternating natural / decimated groups and the length is a multiple of 512 samples (every
 * shipped configuration), except for five to seven 4.8 s utterances per call, where the per-layer launches measured 1 %
 * ahead; 0 when every layer (or layer pair) is a launch of its own. */
WN_API int wn_iaf_layer_groups(const wn_handle* h, int B, int F);

/* Launch structure of the hoisted form for this handle: mode 1 = layer groups at every call size they support, -1 = never
 * (one launch per layer or layer pair), 0 = back to what the handle was created with (the size policy above, or the form
 * the environment variables WN_GROUPS=1 / WN_NO_GROUPS=1 named when wn_create read them -- ONCE).  A switch (see
 * "Concurrency"): WN_ESTATE while another thread's work call is inside the library; cross-form tests and A/B runs use it
 * between calls.  Returns WN_EINVAL for any other mode. */
WN_API int wn_iaf_set_groups(wn_handle* h, int mode);

/* MEASUREMENT ONLY: aid used by bench.py (not part of the reference's surface; a switch in the sense of
 * "Concurrency" above).  Between begin and end, wn_iaf_generate records a hipEvent pair
 * on the caller's stream around every flow's run of residual-stack launches --
 * whatever form the call takes: iaf_group_kernel (layer groups, the default of small
 * calls), iaf_layer_c_kernel / iaf_pair_c_kernel (one / two layers per launch),
 * iaf_layer_h_kernel (fused form), iaf_layer_kernel (fp32 form).  wn_profile_end
 * synchronises those events and returns the summed elapsed milliseconds and the
 * number of launches they bracket: average launch duration = layer_ms / layer_launches.
 * Every recorded event costs the stream a bubble of a few microseconds, so
 * wn_profile_pause(h, 1) suspends the recording for the following calls (0 resumes):
 * bench.py samples every few steps of its timed region instead of all of them. */
WN_API int wn_profile_begin(wn_handle* h);
WN_API int wn_profile_pause(wn_handle* h, int paused);
WN_API int wn_profile_end(wn_handle* h, double* layer_ms, int64_t* layer_launches);

/* MEASUREMENT ONLY: second mode, same caveats: between parts_begin and parts_end every wn_iaf_generate records one hipEvent on
 * the caller's stream where a PART of the call begins -- 0: prologue + epilogue (pads, noise draw, final clip/quantise),
 * 1: mel upsampler, 2: conditioning GEMM (hoisted form), 3: residual stack (start convs, layers / layer groups, flow
 * heads).  parts_end synchronises and returns the summed milliseconds per part (part_ms[WN_PROFILE_PARTS]) and the
 * number of calls recorded: bench.py's in-process replacement for a replayed rocprofv3 kernel trace.  Each event costs
 * the stream a bubble of a few microseconds, so the sum of the parts is slightly above the unprofiled call time. */
#define WN_PROFILE_PARTS 4
WN_API int wn_profile_parts_begin(wn_handle* h);
WN_API int wn_profile_parts_end(wn_handle* h, double* part_ms, int64_t* calls);

/* MEASUREMENT ONLY (package power of one part of the call, scripts/dev_power.py) -- a restricted call SKIPS WORK and its
 * results are meaningless, so the switch cannot be left armed: it is accepted only between wn_profile_parts_begin and
 * wn_profile_parts_end (WN_ESTATE otherwise), and parts_end (like parts_begin and wn_destroy) puts the handle back to "every
 * part".  While armed, the following wn_iaf_generate calls of the split-fp16 / fp32 student paths run only the parts whose
 * bits are set in mask (bit k = part k above; 15 = everything) -- e.g. a loop of conditioning GEMMs alone; the skipped parts
 * leave their buffers as the last full call wrote them.  At most 4096 part events are kept per session (a long power loop
 * stops recording, the restriction stays).  WN_EINVAL for a mask outside 1..15. */
WN_API int wn_profile_parts_only(wn_handle* h, int mask);

/* Message of the calling thread's last failed call (any handle, or wn_create).  `h` is accepted for source compatibility
 * and ignored: the text is thread-local, so concurrent callers never see -- or tear -- each other's messages. */
WN_API const char* wn_last_error(const wn_handle* h);

WN_API void wn_destroy(wn_handle* h);

/* CRC32C (Castagnoli) of n host bytes, continuing from `crc` (0 to start): the checksum of the TensorFlow V2 checkpoint
 * bundle (nsynth_wavenet_amd/tf_bundle.py reads and writes `model.ckpt-N.index` / `.data-*` with it; the reference leaves
 * this to tf.train.Saver, wavenet/fastgen.py:80-84).  Host-only helper, needs no handle and no device. */
WN_API uint32_t wn_crc32c(const void* data_host, size_t n, uint32_t crc);

#ifdef __cplusplus
}
#endif
#endif /* WNHIP_H_ */
