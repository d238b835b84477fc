/* bvcodec.h - C ABI of libbvcodec_hip.so: the MI355X (gfx950) implementation of the
 * BVRNNCodecModel encode/decode hot path.
 *
 * The reference (BenjSta/bernoulli-var-speech-codec) is pure Python/PyTorch and has NO FFI of its
 * own; its boundary for this path is the Python class BVRNNCodecModel (bvrnn_codec_model.py:19-76).
 * This header is the boundary the build adds underneath that class: each entry point names the
 * reference call it replaces (file:line relative to the reference checkout).  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C, no torch/HIP types: `stream` is a hipStream_t passed as void* (NULL = default stream);
 *  - every pointer named d_* is DEVICE memory owned by the caller, contiguous float32;
 *    every pointer named h_* is HOST memory;
 *  - the compute entry points (bvc_stft_logmel, bvc_bvrnn_*, bvc_bigvgan, bvc_encode, bvc_decode, bvc_decode_conceal,
 *    bvc_encode_ragged, bvc_decode_ragged, bvc_vocoder_stream_push, bvc_pack/unpack_codes, bvc_resample_poly, bvc_peak_normalize, bvc_resampler_push / push_multi / flush) are
 *    asynchronous on `stream` and use only the caller-provided workspace.  They do not allocate or
 *    synchronise, with these exceptions: the first calls per process create a handful of HIP events (the
 *    persistent launches' ticket, the end-of-call mark of the "auto" schedule, one per bvc_flow_fence slot in
 *    use), the launch-per-layer schedule captures and instantiates a hipGraph on a stream of the library's own
 *    on the first call per (batch, workspace), and the call that follows a reported time-out re-runs the
 *    residency census (it synchronises a stream of the library's own, and the device if the census fails);
 *  - capturing into a graph of your own: allowed for every compute entry point.  While `stream` is
 *    being captured a call records no event and waits on none, and its recurrence takes the
 *    launch-per-layer kernels, launched directly into your capture (the persistent recurrence kernel is
 *    never captured: see "recurrence" below); the status word is still read when the call is ISSUED, not
 *    on replay;
 *  - bvc_model_status, bvc_probe_end, bvc_kprobe_* and the bvc_test_* helpers synchronise the device
 *    (bvc_model_poll_status does not);
 *  - return value: 0 = BVC_OK, negative = error code; bvc_last_error() gives the text
 *    (thread-local); no C++ exception crosses the boundary;
 *  - one in-flight call per (model, workspace): calls on different streams with different
 *    workspaces may overlap (persistent recurrence kernels of overlapping calls run one after the
 *    other, everything else concurrently; with the default "recurrence" = auto overlapping calls take
 *    the launch-per-layer schedule, whose kernels interleave).  Several host threads may issue calls on ONE model
 *    at once, each with its own workspace and stream (the model's graph cache, the persistent launches' ticket and
 *    the census are guarded inside the library); a model's weights are immutable after creation, and its options
 *    (bvc_model_set_option) must not be changed while another thread is issuing calls on it.
 */
#ifndef BVCODEC_H
#define BVCODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BVC_ABI_VERSION 3   /* 2: + bvc_model_get_option, bvc_flow_fence, bvc_kprobe_read_span; recurrence option takes 2 (auto); status word reported by every compute entry
                             * 3: + bvc_model_poll_status, bvc_forward
                             *    still 3 (new symbols only, nothing existing changed): + bvc_encode_ragged, bvc_decode_ragged;
                             *    + bvc_stream_codec_open / close / set_bits / slot_frames;
                             *    + bvc_stream_codec_create_dir / packets / tick_recv / finish / slot_state;
                             *    + bvc_bvrnn_decode_conceal, bvc_decode_conceal, bvc_stream_codec_set_conceal;
                             *    + bvc_resampler_*;
                             *    + bvc_resampler_create_multi / set_taps_rate / open_rate / push_multi */

enum {
    BVC_OK = 0,
    BVC_EINVAL = -1,      /* bad argument / unsupported shape */
    BVC_ENOMEM = -2,      /* workspace too small or device allocation failed */
    BVC_EHIP = -3,        /* HIP runtime error (see bvc_last_error) */
    BVC_EMISSING = -4,    /* a required weight tensor is missing or has the wrong size */
    BVC_ENODEVICE = -5,   /* no gfx950 device visible */
    BVC_ETIMEOUT = -6     /* a persistent recurrence kernel gave up waiting for its peers (bvc_model_status) */
};

/* Static description of the codec; mirrors the TOML keys the reference facade reads
 * (configs/config_varBitRate.toml:21-29,35-37,39-56; bvrnn_codec_model.py:27-36,49-59).
 * The generator's width: upsample_initial_channel is 16, 32, 64, 128, 256 or 512 and halves at every upsampling stage; every stage has
 * at least 8 channels and conv_post reads 8, 16 or 32 (bvc_model_create returns BVC_EINVAL otherwise).  Stages of 128 and 256
 * channels - the first one or two of a generator of 256 / 512 - run as causal, unfiltered, fused AMP pairs only: "layers_sym" or
 * "layers_antialias" set on such a stage, or BVC_UNFUSED_AMP=1 with such a model, is BVC_EINVAL at creation; a stage of 256 (128)
 * channels takes at most 2^31 / 1024 (2^31 / 512) - 512 rows per item.  Everything else - streaming, mixed lengths, concealment, the
 * switches on the stages of 64 channels and fewer - works at every width. */
typedef struct bvc_config {
    int32_t num_mels;          /* 80 */
    int32_t h_dim;             /* 1024 */
    int32_t z_dim;             /* 64 */
    int32_t var_bit;           /* 1: variable bits/frame mask (bvrnn.py:180-182,193-194) */
    int32_t n_fft;             /* 1024 (== win) */
    int32_t hop;               /* 256 */
    int32_t pad_left;          /* mel_pad_left = 256 */
    int32_t sample_rate;       /* 22050 */
    float   fmin, fmax;        /* 0, 8000 */
    int32_t upsample_initial_channel;      /* 128 (16 .. 512, powers of two) */
    int32_t n_up;                          /* 4 */
    int32_t up_rates[8];                   /* 8,8,2,2 */
    int32_t up_kernels[8];                 /* 16,16,4,4 (must be 2*rate) */
    int32_t n_resk;                        /* 3 */
    int32_t res_kernels[4];                /* 3,7,11 */
    int32_t res_dilations[4][3];           /* 1,3,5 each */
} bvc_config;

/* One named HOST tensor (float32, contiguous, PyTorch layout).  Names are the reference's
 * state_dict keys: BVRNN (bvrnn.py:30-83) "mean_mel","std_mel","phi_x.0.weight",...,
 * "rnn.bias_hh_l0"; generator (models.py:132-205) with weight-norm ALREADY FOLDED by the caller:
 * "conv_pre.weight","conv_pre.bias","ups.0.1.weight",...,"resblocks.0.convs1.0.weight",...,
 * "resblocks.0.activations.0.alpha",...,"activation_post.alpha","conv_post.weight",...;
 * plus "mel_basis" (num_mels x (n_fft/2+1), the librosa.filters.mel matrix of meldataset.py:68).
 *
 * Anti-aliased activations (vocoder_config.layers_antialias / antialias_post, models.py:69-93,172-192): two optional tensors say where
 * the generator wraps its SnakeBeta in Activation1d (alias_free_torch/act.py:8-28) - "layers_antialias", n_up values, non-zero = every
 * activation of that stage's AMP blocks; "antialias_post", one value, activation_post.  bvc_config keeps its layout.  A flagged
 * activation NAME ("resblocks.K.activations.J", "activation_post") is read from the reference's keys of that module: "NAME.act.alpha",
 * "NAME.act.beta", "NAME.upsample.filter", "NAME.downsample.lowpass.filter" (12 values each, the ones the reference convolves with);
 * an unflagged one from "NAME.alpha" / "NAME.beta".  Tensors of the other layout are BVC_EMISSING either way.
 * bvc_bigvgan, bvc_decode, bvc_forward, bvc_decode_conceal and bvc_test_vocoder_layer / _tap (window == 0) work unchanged for such a
 * model.  What counts on the generator being causal returns BVC_EINVAL for it - bvc_vocoder_stream_create, bvc_stream_codec_create
 * (bvc_stream_codec_create_dir unless BVC_STREAM_SEND), bvc_decode_ragged, bvc_test_vocoder_layer with window != 0: a filtered
 * activation reads 5 rows ahead, an AMP block 30, so every output sample depends on later frames - about 53 ms of look-ahead when all
 * four stages and the post activation are filtered (30 rows at each of 8 / 64 / 128 / 256 rows per frame, and 5 samples).
 *
 * Symmetric layers (vocoder_config.layers_sym / pre_sym / post_sym, models.py:35-44,151-155,209-213,230-233): three more optional tensors -
 * "layers_sym", n_up values, non-zero = upsampler i is ConvTranspose1d(padding = (k-u)/2) and the stage's AMP blocks pad both sides;
 * "pre_sym" and "post_sym", one value each, conv_pre / conv_post pad [3, 3] instead of [6, 0].  They add no weight tensors and bvc_config
 * keeps its layout.  A symmetric upsampler makes L * rate rows instead of (L + 1) * rate: bvc_vocoder_length(m, T) follows.  A stage that
 * is symmetric and anti-aliased, post_sym with antialias_post, an even resblock kernel size on a symmetric stage and a symmetric stage
 * with BVC_UNFUSED_AMP set are BVC_EINVAL from bvc_model_create.  The same entry points as above work for such a model and the same
 * ones return BVC_EINVAL (bvc_last_error() says "symmetric" unless the model is filtered too).  A symmetric layer reads as many rows
 * ahead as behind, a bounded number: bvc_vocoder_stream_create_lookahead runs such a generator incrementally behind that delay (a
 * filtered one stays refused there too). */
typedef struct bvc_tensor {
    const char  *name;
    const float *h_data;
    int64_t      numel;
} bvc_tensor;

typedef struct bvc_model bvc_model;     /* opaque: device-resident, re-laid-out weights */

int          bvc_abi_version(void);
const char  *bvc_last_error(void);

/* Replaces BVRNNCodecModel.__init__'s module construction + load_state_dict
 * (bvrnn_codec_model.py:30-42): uploads and re-lays-out the weights on the current device. */
int  bvc_model_create(const bvc_config *cfg, const bvc_tensor *tensors, int32_t n_tensors,
                      bvc_model **out);
void bvc_model_destroy(bvc_model *m);

/* Run-time options of a model (not thread-safe; set them while no call is in flight).
 *   "recurrence": how the frame loop of BVRNN.encode / BVRNN.decode (bvrnn.py:186-206, 222-227) is scheduled.
 *                 0 = one persistent kernel launch per call (fastest for one batch at a time),
 *                 1 = one launch per layer, hipGraph-replayed (more throughput when batches are in flight on several streams),
 *                 2 = automatic (default; the start-up default follows BVC_RECURRENCE=persistent|layers|auto): persistent while
 *                     calls come one at a time; while a call starts before the previous one - issued on ANOTHER stream - has
 *                     finished, launch per layer, for all streams alike.
 *                 Whatever the option says, a call takes the launch-per-layer kernels when its stream is being captured
 *                 into a graph (a persistent launch is serialised against other persistent launches by a host-side ticket,
 *                 which a replay would skip), when the batch is beyond the persistent kernel's limits, or when the
 *                 residency census at bvc_model_create found that a full persistent grid is not co-resident on this device.
 *   "vocoder_full_tiles": 1 (default) = the eight-channel generator stage runs on the kernel that packs two output rows into
 *                 one MFMA tile, 0 = on the generic kernel (half of every tile is channel padding).  Same bits either way;
 *                 a validation switch (per model, like every option).
 *   "vocoder_c16_kernel": 1 (default) = the sixteen-channel generator stage runs offline on its persistent kernel (weights in
 *                 registers, next tile's rows under the current tile's convs, 16-byte epilogues), 0 = on the generic kernel.
 *                 Same bits either way; per model.
 *   "decode_fold": 1 (default) = the persistent DECODE kernel runs phi_x.0((dec.6(u) - mean) / std) - three maps with no
 *                 non-linearity between them (bvrnn.py:80, :226) - as ONE affine map of u (folded in float64 at model creation):
 *                 one wide layer instead of two narrow hops per frame; dec.6(u), the decoder's output, is then one batched GEMM
 *                 over the kept u of all frames.  mel^ / h_T agree with the layer-by-layer program to rounding (2e-5 / 5e-6 in
 *                 the tests); 0 = the layers as the reference lists them.
 *   "encode_fold": 1 (default) = the same fold in the persistent ENCODE kernel (dec.6's output is not needed there).  The
 *                 folded layer feeds the next state and so the next codes: the same function with another rounding, like
 *                 another order of summation - the goldens and the full-size parity runs give the same bits either way
 *                 (tests/test_gpu_robustness.py compares both settings); 0 = the layers as the reference lists them.
 *   "flow_spin_limit" (polls before a wait inside the persistent kernel gives up; default 4,000,000, more than a second),
 *   "flow_debug_withhold" (1: workgroup 0 of every persistent launch does nothing, so its consumers time out),
 *   "flow_debug_nofill" (1: the plain layer program without filler quanta): test switches.
 * bvc_model_get_option reads "recurrence", "decode_fold", "encode_fold", "flow_resident" (1: the census found a full persistent grid co-resident),
 * "flow_supported" (1: h_dim / z_dim / num_mels are laid out for the persistent kernel), "compute_units". */
int bvc_model_set_option(bvc_model *m, const char *name, int32_t value);
int bvc_model_get_option(const bvc_model *m, const char *name, int32_t *value);

/* The persistent recurrence kernel's workgroups hand activations to each other, so all of them must be resident together;
 * every wait in it is bounded.  If a wait ever times out (a workgroup that never became resident: another process on the
 * device, a CU mask), the kernel still ends, with invalid results, and stores a code (frame << 4 | layer, top bit set) in a
 * status word in host-mapped memory.  EVERY compute entry point (bvc_encode, bvc_decode, bvc_*_ragged, bvc_bvrnn_*, bvc_bigvgan,
 * bvc_stft_logmel) reads that word first, without synchronising, and returns BVC_ETIMEOUT - once, clearing it - if an
 * earlier call of this model timed out.  bvc_model_status synchronises the device first, so it also sees calls still in
 * flight; it returns BVC_ETIMEOUT and the code, and clears it; BVC_OK and 0 otherwise. */
int bvc_model_status(const bvc_model *m, uint32_t *code);
/* The same check WITHOUT synchronising: for a caller that has just synchronised by its own means - a blocking device-to-host copy
 * of a call's output, hipStreamSynchronize - and wants to know whether THAT call was valid instead of learning it from the next
 * one.  (bvcodec/model.py calls it behind every copy of an output to a CPU tensor.)  After any report of a time-out the residency
 * census of bvc_model_create runs again before the model's next persistent launch: a tenant that arrived on the device later
 * moves the model to the launch-per-layer schedule instead of letting every call time out. */
int bvc_model_poll_status(const bvc_model *m, uint32_t *code);

/* A persistent recurrence launch needs every compute unit of the device.  Work of the caller's own that holds compute units
 * for an unbounded time - above all an RCCL collective, whose kernel waits for its peers - must not be running beside it.
 * bvc_flow_fence(stream) marks the work issued on `stream` so far: the next persistent launch of this process on the current
 * device (any model, any stream) starts only after it has finished.  Cheap (one event record); not needed when the
 * collective and the codec calls share one stream.  bvcodec/dist.py calls it behind every gather. */
int bvc_flow_fence(void *stream);

/* Frames for L samples: floor(L / hop)  (torch.stft center=False after the reflect pad,
 * meldataset.py:72-85).  Returns < 0 when L <= win - hop (reflect pad impossible). */
int64_t bvc_num_frames(const bvc_model *m, int64_t L);
/* Un-trimmed vocoder output length for T frames: 256*T + 294 for the shipped config
 * (models.py:216-217 applied four times with padding=0). */
int64_t bvc_vocoder_length(const bvc_model *m, int64_t T);
/* Bytes of caller-provided device workspace needed by any entry point at batch B, T frames. */
size_t  bvc_workspace_bytes(const bvc_model *m, int32_t B, int64_t T);

/* mel_spectrogram(y*scale, ...) of meldataset.py:60-95 as called at bvrnn_codec_model.py:49-56,
 * including the .permute(0,2,1): d_wav (B,L) -> d_mel (B,T,num_mels), natural-log mel. */
int bvc_stft_logmel(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale,
                    float *d_mel, void *stream);

/* BVRNN.encode (bvrnn.py:163-209).  d_mel (B,T,num_mels); d_bits (B,T) bits per frame (ignored
 * when var_bit=0); d_h0 (B,h_dim) or NULL for zeros.  Outputs: d_codes (B,T,z_dim) in {0,1,0.5};
 * optional d_all_h (B,T,h_dim) = state BEFORE each frame (bvrnn.py:205); optional d_hT (B,h_dim) =
 * state after the last frame; optional d_prob (B,T,z_dim) = sigmoid output before rounding. */
int bvc_bvrnn_encode(const bvc_model *m, const float *d_mel, const float *d_bits, const float *d_h0,
                     int32_t B, int64_t T, float *d_codes, float *d_all_h, float *d_hT,
                     float *d_prob, void *d_ws, size_t ws_bytes, void *stream);

/* BVRNN.decode (bvrnn.py:211-229).  d_codes (B,T,z_dim) -> d_mel (B,T,num_mels), d_hT optional. */
int bvc_bvrnn_decode(const bvc_model *m, const float *d_codes, const float *d_h0, int32_t B,
                     int64_t T, float *d_mel, float *d_hT, void *d_ws, size_t ws_bytes,
                     void *stream);

/* BVRNN.decode that conceals lost frames from the model's prior net (bvrnn.py:68-73; not in the reference, whose decoder has no notion of
 * a lost frame).  d_present (B,T) uint8 marks the frames of d_codes (B,T,z_dim) that arrived.  Per row, with state h_t (h_0 = d_h0 or
 * zeros), frame t:  p_t = prior(h_t), sigmoid included;  g_t = round-half-even(p_t), on a var_bit model 0.5 at positions >= d_bits[b,t]
 * (bvrnn.py:193-194; d_bits (B,T), NULL unless var_bit; a fixed-rate model generates all z_dim bits);  z_t = present ? codes[b,t] : g_t;
 * then phi_z, dec, phi_x((dec - mean) / std) and the GRU exactly as bvrnn.py:223-227.  z_t is a SELECT: whatever a lost position of
 * d_codes holds - garbage, NaN, Inf - reaches nothing.  Outputs: d_mel (B,T,num_mels); optional d_hT (B,h_dim); optional d_codes_out
 * (B,T,z_dim) = z_t, the codes with the gaps filled (may be d_codes itself); optional d_prior (B,T,z_dim) = p_t of EVERY frame.
 * The result is a function of (codes, present, bits, h0) alone: the call runs ONE program on all its frames, lost or not, on every
 * schedule (persistent, launch per layer, captured), so it does not depend on batching or on where a sequence is cut into calls
 * (carry d_hT into the next call's d_h0).  That program cannot batch phi_z over all frames - a frame's codes exist only inside the frame
 * - so it sums dec.0 and the GRU's input gates in BVRNN.encode's order, the h half before the phi_z half.  With every frame present it
 * therefore agrees with bvc_bvrnn_decode to rounding, not bit for bit: the difference bvc_forward has against bvc_encode + bvc_decode
 * (mel^ / h_T within 2e-5 / 5e-6 in the tests).  "decode_fold" applies.  BVC_EMISSING on a model created without prior.{0,2,4}.*. */
int bvc_bvrnn_decode_conceal(const bvc_model *m, const float *d_codes, const uint8_t *d_present, const float *d_bits,
                             const float *d_h0, int32_t B, int64_t T, float *d_mel, float *d_hT, float *d_codes_out,
                             float *d_prior, void *d_ws, size_t ws_bytes, void *stream);

/* BVRNN.forward (bvrnn.py:86-160), forward VALUES only (their gradients: bvc_bvrnn_backward below): the training-time pass with the
 * stochastic Bernoulli sampler round(u - 0.5 + p), the prior net and the KL term.
 *   d_mel (B,T,num_mels), d_bits (B,T) (NULL unless var_bit);
 *   h_use_gen: HOST array of T bytes, use_gen[t] = (random_num_t < p_use_gen), bvrnn.py:111-120: frame t is
 *     conditioned on h2 (the state fed with generated features) when set, else on h (teacher-forced);
 *   update_h = (p_use_gen < 1), update_h2 = (p_use_gen > 0)  (bvrnn.py:142-145);
 *   d_noise (B,T,z_dim) uniform [0,1) samples, or NULL for greedy=True (bvrnn.py:123-126);
 *   outputs: d_dec (B,T,num_mels) = all_dec_mean, d_kld (T) = per-frame KLD terms (the reference returns their
 *   mean, bvrnn.py:160); optional d_z (forward value of z_t, i.e. round(.) - p + p, masked), d_prob (enc_t),
 *   d_prior (prior_t), each (B,T,z_dim).  Needs the prior.{0,2,4}.{weight,bias} tensors at bvc_model_create. */
int bvc_bvrnn_forward(const bvc_model *m, const float *d_mel, const float *d_bits,
                      const uint8_t *h_use_gen, int32_t update_h, int32_t update_h2,
                      const float *d_noise, int32_t B, int64_t T, float *d_dec, float *d_kld,
                      float *d_z, float *d_prob, float *d_prior, void *d_ws, size_t ws_bytes,
                      void *stream);

/* The backward pass of bvc_bvrnn_forward: the vector-Jacobian product of BVRNN.forward at d_gdec (B,T,num_mels), the gradient of a loss
 * with respect to all_dec_mean, and g_kld, its gradient with respect to the scalar kld the reference returns (the mean of d_kld).  The
 * sample is differentiated as the reference does (bvrnn.py:124,126: straight through, d z / d enc_t = the bit mask), the KLD's clips
 * as torch.clip does.  Inputs as bvc_bvrnn_forward; the call runs its own forward - the launches of bvc_bvrnn_forward, every frame
 * kept - so d_dec, d_kld, d_z, d_prob, d_prior (all optional here) are that call's bits.
 *   d_grads: bvc_bvrnn_grad_layout's `total` floats, OVERWRITTEN (never accumulated into): the gradient of every trainable BVRNN
 *     tensor in its state-dict layout (weight (out, in), bias (out), rnn.weight_ih_l0 (3H, 2H), ...).  mean_mel / std_mel are not
 *     trainable and log_sigma does not enter the pass: they have no entry.
 *   d_gmel (B,T,num_mels), optional: the gradient with respect to d_mel.
 * f32 throughout, no atomics: the order of every sum is a function of the shapes alone, two calls give the same
 * bits.  Workspace: bvc_bvrnn_backward_workspace_bytes(m, B, T) - the tape and every layer's gradient of all frames, about 70 (B T
 * h_dim) floats.  The first call on a model uploads the transposed weights (or bvc_bvrnn_backward_prepare does, which synchronises the
 * stream; needed before a call is captured into a graph); a model that never calls either allocates nothing.  Refusals as
 * bvc_bvrnn_forward, with its messages: BVC_EMISSING without the prior.* tensors; BVC_EINVAL for z_dim > h_dim, var_bit without
 * d_bits, no state updated, a frame conditioned on a state that is never updated; BVC_ENOMEM for a short workspace.  The call leaves
 * the model's weights alone; bvc_optimizer_step (below) takes d_grads and updates them in place. */
int bvc_bvrnn_backward(const bvc_model *m, const float *d_mel, const float *d_bits, const uint8_t *h_use_gen, int32_t update_h,
                       int32_t update_h2, const float *d_noise, int32_t B, int64_t T, const float *d_gdec, float g_kld,
                       float *d_grads, float *d_gmel, float *d_dec, float *d_kld, float *d_z, float *d_prob, float *d_prior,
                       void *d_ws, size_t ws_bytes, void *stream);
size_t bvc_bvrnn_backward_workspace_bytes(const bvc_model *m, int32_t B, int64_t T);
int bvc_bvrnn_backward_prepare(const bvc_model *m, void *stream);
/* Where every gradient is in d_grads, for a model of this configuration (host arithmetic only: needs no GPU): entry i is the tensor names[i] (its state-dict key; the strings live as long as the library) of
 * numels[i] floats at float offset offsets[i].  *count = the entries (36), *total = the floats of d_grads.  names / offsets / numels
 * may be NULL (to ask for count and total); otherwise each has room for `capacity` entries, BVC_EINVAL if that is too few. */
int bvc_bvrnn_grad_layout(const bvc_config *cfg, const char **names, int64_t *offsets, int64_t *numels, int32_t capacity, int32_t *count,
                          int64_t *total);

/* The trainable tensors of a LIVE model as one flat device buffer in bvc_bvrnn_grad_layout order (`total` floats, 16-byte aligned).
 * bvc_bvrnn_params_get gathers the values the model holds.  bvc_bvrnn_params_set rewrites, in place and stream-ordered, every form of
 * the weights the model's kernels read - natural, fragment-packed and gate-interleaved copies, the float64 fold of dec.6 -> norm ->
 * phi_x.0 (computed on the device with the host's operations, the same bits), and the transposed copies of the backward pass once they
 * exist - at the addresses they already have: the next encode, decode, forward or backward on any schedule, a captured graph included,
 * runs on the new values, and the model is then BIT FOR BIT the one bvc_model_create builds from them.  No host synchronisation, no host
 * copy, no new model.  mean_mel / std_mel are read by the fold and never written.  The first bvc_bvrnn_params_set (or bvc_optimizer_step)
 * on a model allocates the model's flat float32 master copy of the parameters (not inside a stream capture); a model that calls none of
 * this allocates nothing.  Like the model options, a rewrite is ordered on ITS stream only: a call in flight on another stream while the
 * weights change is the caller's to serialise.  BVC_EMISSING without the prior.* tensors. */
int bvc_bvrnn_params_get(const bvc_model *m, float *d_params, void *stream);
int bvc_bvrnn_params_set(bvc_model *m, const float *d_params, void *stream);

/* AdamW (torch.optim.AdamW without amsgrad and maximize; weight_decay = 0: Adam) on a live model's parameters, everything on the device.
 * The optimiser owns exp_avg and exp_avg_sq (`total` floats each, zero at creation) and the step count; the master copy of the
 * parameters belongs to the model (above), so bvc_bvrnn_params_set followed by a step starts from the values that were set.  Destroy the
 * optimiser before its model.
 * bvc_optimizer_step: d_grads = the flat buffer bvc_bvrnn_backward writes (read, never written).  Per element, in f32, in this order and
 * every operation rounded on its own, with t the count of this step, bc1 = 1 - beta1^t and bc2 = 1 - beta2^t computed in double:
 *     p *= 1 - lr weight_decay;  m = beta1 m + (1 - beta1) g;  v = beta2 v + ((1 - beta2) g) g;
 *     p -= (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
 * max_grad_norm > 0: g is first scaled by min(1, max_grad_norm / (norm + 1e-6)), norm the 2-norm of ALL of d_grads
 * (torch.nn.utils.clip_grad_norm_).  The norm is summed in float64 in two stages over fixed chunks, without atomics: two calls give the
 * same bits; the update reads the factor from device memory (no host synchronisation).  d_grad_norm (optional, one device float)
 * receives the unclipped norm.  The step ends with the rewrite of bvc_bvrnn_params_set from the new values.  The hyperparameters are
 * passed with every step: a schedule is the caller's.  BVC_EINVAL for lr < 0, a beta outside [0, 1), eps <= 0, weight_decay < 0, a null
 * argument or a stream that is being captured (the scalars change with every step). */
typedef struct bvc_optimizer bvc_optimizer;
typedef struct bvc_adamw_config { double lr, beta1, beta2, eps, weight_decay, max_grad_norm; } bvc_adamw_config;
int bvc_optimizer_create(bvc_model *m, bvc_optimizer **out);
void bvc_optimizer_destroy(bvc_optimizer *opt);
int bvc_optimizer_step(bvc_optimizer *opt, const bvc_adamw_config *cfg, const float *d_grads, float *d_grad_norm, void *stream);
/* The optimiser's state, for checkpoints: the step count and the two moments (`total` floats each, device memory; any of the three
 * may be NULL). */
int bvc_optimizer_state_get(const bvc_optimizer *opt, int64_t *step, float *d_exp_avg, float *d_exp_avg_sq, void *stream);
int bvc_optimizer_state_set(bvc_optimizer *opt, const int64_t *step, const float *d_exp_avg, const float *d_exp_avg_sq, void *stream);
/* tests: the folded hop px0_dec3 as the model holds it, d_w (h_dim, h_dim) unpacked to its natural layout and d_b (h_dim) */
int bvc_test_folded_hop(const bvc_model *m, float *d_w, float *d_b, void *stream);

/* BigVGAN.forward(x, length) (models.py:207-238) followed by `/ out_scale_div`
 * (bvrnn_codec_model.py:71: .squeeze(1) / SCALING).  d_mel is TIME-major (B,T,num_mels), i.e. what
 * bvc_bvrnn_decode emits (the reference permutes to (B,80,T) first).  d_wav (B, n_out) with
 * n_out = min(length, bvc_vocoder_length(T)). */
int bvc_bigvgan(const bvc_model *m, const float *d_mel, int32_t B, int64_t T, int64_t length,
                float out_scale_div, float *d_wav, void *d_ws, size_t ws_bytes, void *stream);

/* Incremental BigVGAN for streaming (not in the reference, whose BigVGAN.forward, models.py:207-238,
 * always sees the whole utterance).  The state keeps the last rows of every activation tensor of the
 * generator for B parallel streams; bvc_vocoder_stream_push runs the generator over only the k new mel
 * frames d_mel (B,k,num_mels) and writes exactly their samples d_wav (B, k*prod(upsample_rates)),
 * equal to the corresponding slice of bvc_bigvgan over the whole utterance.  One in-flight push per
 * state; state buffers are allocated by create (device memory), zeroed by create/reset. */
typedef struct bvc_vocoder_stream bvc_vocoder_stream;
int bvc_vocoder_stream_create(const bvc_model *m, int32_t B, int32_t max_frames_per_push,
                              bvc_vocoder_stream **out);
void bvc_vocoder_stream_destroy(bvc_vocoder_stream *st);
int bvc_vocoder_stream_reset(bvc_vocoder_stream *st, void *stream);
int bvc_vocoder_stream_push(bvc_vocoder_stream *st, const float *d_mel, int32_t k, float out_scale_div,
                            float *d_wav, void *stream);

/* The same behind a look-ahead window, for generators with symmetric layers (and for causal ones).  A symmetric generator is not
 * causal, but its look-ahead is bounded: sample t is final once frame (t + D) / hop has arrived, D = bvc_vocoder_lookahead(m) - 0
 * for a causal model, 3258 samples (148 ms) when every layer of the shipped geometry is symmetric, < 0 for a model that cannot
 * stream (anti-aliased activations).  On a state made by bvc_vocoder_stream_create_lookahead, bvc_vocoder_stream_push writes the
 * samples that BECAME final with its k frames - [max(0, hop n_old - D), max(0, hop n_new - D)), dense (B, that many), possibly none
 * (d_wav may then be NULL) - and bvc_vocoder_stream_flush writes the rest up to bvc_vocoder_length(m, n) with the offline rules of
 * the signal's end; after it only bvc_vocoder_stream_reset is legal (push and flush: BVC_EINVAL).  A flush without frames writes
 * nothing.  bvc_vocoder_stream_samples says how many samples per row the next push of k frames (1 <= k <= max_frames_per_push) or,
 * k == -1, the flush writes: host arithmetic, no synchronisation.  The pushes and the flush, concatenated, equal bvc_bigvgan over the
 * whole mel bit for bit, however the frames are cut into pushes.  For a causal model every push is the plain state's and the flush
 * is the (L + 1) u tail behind hop * n (294 samples).  An anti-aliased model is BVC_EINVAL. */
int64_t bvc_vocoder_lookahead(const bvc_model *m);
int bvc_vocoder_stream_create_lookahead(const bvc_model *m, int32_t B, int32_t max_frames_per_push,
                                        bvc_vocoder_stream **out);
int64_t bvc_vocoder_stream_samples(const bvc_vocoder_stream *st, int32_t k);
int bvc_vocoder_stream_flush(bvc_vocoder_stream *st, float out_scale_div, float *d_wav, void *stream);

/* Whole-hop streaming codec (BASELINE.json configs[4]; not in the reference, which has no streaming mode): B parallel
 * streams, `hop_samples` new samples per stream and tick (e.g. 441 = 20 ms).  A tick runs the front-end for the frames the
 * hop completes (frame t needs samples up to 256 t + 768: 34.8 ms of look-ahead, README.md:19), BVRNN.encode and
 * BVRNN.decode with carried GRU states and the incremental vocoder, i.e. encode + decode of exactly those frames, and equals
 * the offline bvc_encode / bvc_decode of the whole signal on them.  The caller writes the hop into d_in (B, hop_samples)
 * before the tick and finds d_codes (B, n_frames, z_dim) and d_wav (B, n_frames * 256) afterwards (buffers owned by the
 * state, fixed addresses).  Schedule: where the persistent recurrence kernel is available (option "recurrence" not 1, the
 * residency census passed, batch within its range) a tick is launched eagerly with ONE persistent launch per recurrence
 * (BVC_STREAM_FLOW=0 turns that off); otherwise, from the 33rd frame on, a tick of launch-per-layer kernels is replayed from a
 * hipGraph captured on first use (one per frame count and vocoder parity; BVC_STREAM_NO_GRAPH=1 keeps eager launches).  The
 * bits are the same on every schedule.  scale / out_scale_div as in bvc_encode / bvc_decode.  One in-flight tick per state;
 * create allocates, tick does not (except the graph instantiation). */
typedef struct bvc_stream_codec bvc_stream_codec;
int  bvc_stream_codec_create(const bvc_model *m, int32_t B, int32_t hop_samples, float bits_per_frame, float scale,
                             float out_scale_div, bvc_stream_codec **out);
void bvc_stream_codec_destroy(bvc_stream_codec *st);
int  bvc_stream_codec_buffers(bvc_stream_codec *st, float **d_in, float **d_codes, float **d_wav, int32_t *max_frames_per_tick);
int  bvc_stream_codec_tick(bvc_stream_codec *st, int32_t *n_frames, void *stream);

/* Slots: every row of a session is a stream of its own that can be opened, closed, re-used and re-rated while the other rows
 * keep running.  The session still advances in lock step (every tick takes hop_samples for every row and emits the same
 * n_frames for every row); whatever a slot emits is bit for bit what the offline bvc_encode / bvc_decode give for that
 * stream's own signal alone.  bvc_stream_codec_create opens every slot at tick 0 (delay 0); a session on which none of the
 * calls below is made behaves as before.  All four are called BETWEEN two ticks; they are host-side bookkeeping only: they
 * neither launch, allocate nor synchronise, and the next bvc_stream_codec_tick sends what they changed to the device on its own
 * stream, ahead of its own work (one small launch for all changed slots, one more in the tick in which streams start; a
 * tick without changes launches exactly what it launched before).
 *  - open: the samples the caller writes into row `slot` of d_in from the next tick on are samples 0, 1, 2, ... of a new
 *    stream coded with bits_per_frame.  A stream's frame grid is fixed by its sample 0 and the session's by tick 0, so the
 *    library delays the row by a constant *delay_samples (0 <= delay < 256 * max_frames_per_tick; at most 370 for 441-sample
 *    hops), chosen so that the stream's frame 0 is the FIRST frame of a tick.  In that tick, before anything else and for
 *    that row only, the library writes the stream's left reflect padding and zeroes both GRU states and the row's history
 *    in every buffer of the incremental generator.  Frames the session emits for the row before that ("pre-start") belong
 *    to no stream.  After n samples a stream has got (n - delay - 768) / 256 + 1 frames (none while that is negative: the
 *    last `delay` samples are still inside the library).
 *  - close: the row is idle from the next tick on and what the library still holds of the stream (its delayed tail) is
 *    dropped: the stream has got the frames its samples complete, as in a session without slots; the last two frames of
 *    the offline call need the right reflect padding, which bvc_stream_codec_finish (below) writes.  Idle rows ride along in every launch, but
 *    the library never reads d_in for them (it appends zeros): whatever an idle row of d_in holds - uninitialised memory,
 *    Inf, NaN - reaches nothing.  Outputs of idle and pre-start rows are unspecified but finite.
 *  - set_bits: every frame of the row emitted from the next tick on is coded with bits_per_frame; the result equals
 *    bvc_bvrnn_encode with the corresponding per-frame d_bits.  BVC_EINVAL for a model with var_bit = 0.
 *  - slot_frames: which of the last tick's n_frames belong to the slot's stream: [*first, *first + *count), count 0 for an
 *    idle or pre-start slot, and the stream's own index of the first of them.  (Ask before closing the slot.)
 * BVC_EINVAL, with the session untouched: slot out of range, open on an open slot, close / set_bits on an idle one. */
int  bvc_stream_codec_open(bvc_stream_codec *st, int32_t slot, float bits_per_frame, int32_t *delay_samples);
int  bvc_stream_codec_close(bvc_stream_codec *st, int32_t slot);
int  bvc_stream_codec_set_bits(bvc_stream_codec *st, int32_t slot, float bits_per_frame);
int  bvc_stream_codec_slot_frames(bvc_stream_codec *st, int32_t slot, int32_t *first, int32_t *count, int64_t *stream_frame0);

/* Sessions by direction: a tick above is a loopback (encode a row's samples, decode those codes); a deployment runs the two halves
 * in different places with bytes on a wire between them.  bvc_stream_codec_create_dir makes a session that runs ONE half;
 * BVC_STREAM_DUPLEX is bvc_stream_codec_create, launch for launch.  All slot calls work as above in every direction.
 *  - Packets: bvc_stream_codec_packets gives d_packets (B, max_frames_per_tick, bytes_per_frame) uint8 and d_present
 *    (B, max_frames_per_tick) uint8, owned by the session at fixed addresses (both NULL for a duplex session), with
 *    bytes_per_frame = ceil(z_dim / 8) for EVERY row.  Row b's frame holds its nbits_b = min(z_dim, the slot's bits per frame)
 *    leading bits (z_dim for a model with var_bit = 0), bit i in byte i / 8 at position i % 8: the layout of bvc_pack_codes, so
 *    the first ceil(nbits_b / 8) bytes of each frame are what bvc_pack_codes gives for that row.  Frame j of row b of a tick is
 *    at (b * max_frames_per_tick + j) * bytes_per_frame whatever the tick's n_frames.
 *  - BVC_STREAM_SEND: bvc_stream_codec_tick as above on d_in: front-end, BVRNN.encode with the carried state, and the codes
 *    packed into d_packets with each row's own bit count (bytes and bits behind nbits_b are written as 0).  d_codes is filled as
 *    in a duplex session.  No decoder, no generator and no memory for them: bvc_stream_codec_buffers gives NULL for d_wav.
 *    open / close / set_bits / slot_frames: same delays, same frames as a duplex session.
 *  - BVC_STREAM_RECV (hop_samples is ignored; no sample buffer: bvc_stream_codec_buffers gives NULL for d_in): the caller writes
 *    n_frames frames per row into d_packets, marks in d_present which of them arrived (1) and calls bvc_stream_codec_tick_recv
 *    with 1 <= n_frames <= max_frames_per_tick (7: whatever one tick of a send session emits).  The tick unpacks with each row's
 *    bit count, runs BVRNN.decode with the carried state and the incremental vocoder, and leaves d_wav (B, 256 n_frames) (and the
 *    unpacked d_codes).  Bytes and bits behind nbits_b are ignored.  A frame whose d_present byte is 0 is a LOST frame: it is
 *    decoded as a frame of no bits - codes all 0.5, what a variable-rate coder writes and reads at masked positions - whatever
 *    its bytes hold, and the GRU state moves on through it; the result equals bvc_decode of the same code tensor with those frames
 *    set to 0.5.  (A late packet is a lost packet unless the session has a repair window: bvc_stream_codec_set_repair below.  bvc_stream_codec_set_conceal(st, 1) generates lost frames from the
 *    model's prior instead: below.)  Idle rows
 *    are all 0.5 whatever their bytes and d_present hold.  Slots: a receive tick is frame-aligned, so open reports delay 0 and the
 *    stream's frame 0 is the first frame of the next tick, in which - ahead of its own work, for those rows only, in one launch -
 *    h_dec, the row's age and its history in every buffer of the generator are reset.  set_bits changes nbits_b from the next
 *    tick on, close idles the row, slot_frames reports [0, n_frames) for an open row and count 0 for an idle one.
 *    bvc_stream_codec_tick on a receive session and bvc_stream_codec_tick_recv on any other are BVC_EINVAL.
 *  - finish (DUPLEX and SEND; BVC_EINVAL on RECV): the end of a stream, called between two ticks on a running slot in place of
 *    close.  Of the hop the caller writes into the row for the NEXT tick only the first n_last samples (0 <= n_last <=
 *    hop_samples; 0: the stream ended with the previous hop) are the stream's, and they are its last.  With n the stream's
 *    sample count, that tick writes the right reflect padding of the front-end (512 samples x[n - 2 - i], i = 0 .. 511) directly
 *    behind sample n - 1 - nothing of the hop behind n_last is ever used - and from then on the slot is DRAINING: d_in is not
 *    read for it, it rides along in lock step, and this and the following ticks emit its remaining frames up to and including
 *    frame n / 256 - 1; then the slot is idle of its own accord and can be opened again.  slot_frames reports only frames below
 *    that bound (count may be smaller than the tick's n_frames).  The stream has then got ALL bvc_num_frames(n) frames of the
 *    offline bvc_encode (a close leaves it two short); in a duplex session they are decoded like any others.  The up to 294
 *    samples bvc_decode adds behind sample 256 * frames are not part of this.  BVC_EINVAL, session untouched: finish on an idle,
 *    waiting or draining slot, n_last out of range, n <= 512 (too short for the padding); open on a draining slot.  close on
 *    a draining slot drops the rest.
 *  - slot_state: 0 idle, 1 waiting for its frame 0, 2 running, 3 draining.
 * Like the slot calls, finish and slot_state are host bookkeeping between two ticks; the tick that carries a finish out makes one
 * more small launch.  A duplex session on which finish is never called launches exactly what it launched before.
 *  - set_conceal (RECV only; BVC_EINVAL on any other session, BVC_EMISSING on a model without prior.*): what a receive tick does with a
 *    lost frame.  mode 0 (the default): a frame of no bits, as above.  mode 1: the tick runs bvc_bvrnn_decode_conceal with the carried
 *    state - a lost frame of an open row is generated from the prior with the slot's current bit count (set_bits applies; all z_dim
 *    bits when var_bit = 0), idle rows stay all 0.5 - and d_codes holds the FILLED codes afterwards; every stream's samples and codes
 *    equal bvc_decode_conceal of that stream's own packets alone, bit for bit.  Host bookkeeping between two ticks like the slot
 *    calls: it takes effect from the next tick.  A receive session on which it is never called launches exactly what it launched
 *    before. */
enum { BVC_STREAM_DUPLEX = 0, BVC_STREAM_SEND = 1, BVC_STREAM_RECV = 2 };
int  bvc_stream_codec_create_dir(const bvc_model *m, int32_t B, int32_t hop_samples, float bits_per_frame, float scale,
                                 float out_scale_div, int32_t direction, bvc_stream_codec **out);
int  bvc_stream_codec_packets(bvc_stream_codec *st, uint8_t **d_packets, uint8_t **d_present, int32_t *bytes_per_frame);
int  bvc_stream_codec_tick_recv(bvc_stream_codec *st, int32_t n_frames, void *stream);
int  bvc_stream_codec_finish(bvc_stream_codec *st, int32_t slot, int32_t n_last);
int  bvc_stream_codec_slot_state(bvc_stream_codec *st, int32_t slot, int32_t *state);
int  bvc_stream_codec_set_conceal(bvc_stream_codec *st, int32_t mode);

/* Repair window (RECV only; BVC_EINVAL on any other session): a network mostly reorders, and the codec is closed-loop - once the decoder
 * has stepped through a frame with the wrong code its state is no longer the sender's.  With a window of W frames (0 .. 64; 0, the
 * default: off - such a session launches exactly what it launched before and allocates nothing) the session retains, for every tick
 * that holds any of the last W decoded frames, h_dec in front of the tick (taken behind the tick's row starts: a stream that begins
 * with the tick is kept at its zero state) and per (row, frame) of the tick the packet bytes as given, the d_present byte and the bits
 * per frame in force: one more small launch per tick, outside the tick's graph.
 *  - late(slot, stream_frame, packet, taken): the bytes (host memory, bytes_per_frame of them) of ONE frame that a tick was given as
 *    not present; stream_frame counts in the slot's own stream, as slot_frames' stream_frame0 does.  Host bookkeeping between two ticks,
 *    like open / close / set_bits.  *taken = 1 if the slot is running, the frame belongs to its current stream, lies in a retained
 *    tick and is still marked lost.  *taken = 0 - no error, the session untouched - if the frame is older than the window, arrived in
 *    time, was handed in late before, or has not been decoded yet (put it into the next tick), and for an idle or waiting slot.
 *    BVC_EINVAL: a slot out of range, a session that is not a receive session.
 *  - At the head of the next bvc_stream_codec_tick_recv, before that tick's own frames and outside any graph, the packets taken since
 *    the last tick are written into the ring (bytes, present = 1) and every row that got one is decoded again from the retained state
 *    in front of its earliest late frame up to now: tick by tick what the session's ticks ran for those frames, on a compact batch of
 *    those rows - unpacked with the RING's bits per frame, not the slot's current ones; with set_conceal(1) a frame that is still lost
 *    inside the span is generated again, from the repaired state.  Rows with the same first tick share a pass.  The mel frames and
 *    filled codes of a pass are dropped, its last state goes to h_dec and the states in between into the ring, so a second late packet
 *    of the row replays from a repaired state.  Then the tick runs as ever.
 *  - From that tick on the row's filled codes and its state equal, bit for bit, those of a session that was given the packet in time;
 *    its samples equal that session's once the generator's history has flushed, 26 frames later.  Samples already returned are not
 *    touched, other rows never differ.
 *  - set_conceal and set_repair forget what the ring holds (the two recurrence programs agree only to rounding: a frame is replayed by
 *    the program that first decoded it): late packets for frames before such a call are not taken.  close drops what the slot's
 *    stream still had queued.  set_repair allocates the ring and the replay's buffers ((B, W + max_frames_per_tick - 1) frames);
 *    BVC_ENOMEM, the session as before, if they cannot be had; it synchronises the device. */
int  bvc_stream_codec_set_repair(bvc_stream_codec *st, int32_t window_frames);
int  bvc_stream_codec_late(bvc_stream_codec *st, int32_t slot, int64_t stream_frame, const uint8_t *packet, int32_t *taken);

/* Sessions that choose their own rates (SEND, DUPLEX) and that read a bit count per frame (RECV): the closed-loop selection of
 * bvc_bvrnn_encode_vbr(_capped), see there, tick by tick.  The kind of session is decided at creation: its packet buffer has fixed
 * addresses and bvc_stream_codec_packets reports bytes_per_frame = 1 + ceil(z_dim / 8).  A frame has the layout of bvc_pack_codes_vbr -
 * byte 0 its bit count n, then the bits LSB first, then zeros - frame j of row b at (b * max_frames_per_tick + j) * bytes_per_frame as
 * ever; d_sizes (B, max_frames_per_tick) int32 holds 1 + ceil(n / 8), the bytes worth sending, d_bits (same shape, float) holds n.
 *   h_ladder, K: SEND and DUPLEX 1..8 strictly ascending rungs in [0, z_dim]; RECV: NULL, 0.   target: what every slot opens with.
 *   rate_q8, burst_q8: the cap of bvc_bvrnn_encode_vbr_capped, one bucket per row; burst_q8 < 0: no cap.
 *   bits_per_frame: RECV only - the count a lost frame is concealed with (open / set_bits change it per slot); else ignored.
 *  - A SEND tick runs the front-end as ever, then the selection on the tick's (B, k) frames with the carried h_enc, each row's carried
 *    bucket and each row's current target, then one pack launch into d_packets / d_sizes / d_bits; d_codes as ever.  Always on the
 *    launch-per-layer schedule (the candidate rows are not in the persistent kernel); BVC_STREAM_NO_GRAPH=1 gives the same bits.  A stream
 *    equals bvc_encode_vbr(_capped) of its own signal alone, bit for bit.
 *  - A DUPLEX tick is the same followed by the decoder half on the chosen codes (which need no side information); no packet buffer.
 *  - A RECV tick reads n from each present frame's header (above z_dim: z_dim); a frame that is not present has no header and is a frame
 *    of no bits, or with set_conceal(1) generated from the prior at the slot's bits_per_frame.  Behind the unpack the tick is the
 *    receive tick of bvc_stream_codec_create_dir.
 *  - Slots: open on SEND / DUPLEX starts the stream with the session's target, zero state and a full bucket (its bits_per_frame is
 *    ignored); bvc_stream_codec_set_target changes a slot's target from the next tick on; close, finish, slot_frames, slot_state, draining
 *    and idle rows as ever.
 *  - BVC_EINVAL: a fixed-rate model; a bad ladder; burst_q8 >= 0 with rate_q8 < 0 or burst_q8 < ladder[0] * 256; set_bits on SEND /
 *    DUPLEX; set_target on RECV or on a session of the other constructors; set_repair and late (the ring has the fixed wire's width). */
int  bvc_stream_codec_create_vbr(const bvc_model *m, int32_t B, int32_t hop_samples, const int32_t *h_ladder, int32_t K, float target,
                                 int32_t rate_q8, int32_t burst_q8, float bits_per_frame, float scale, float out_scale_div,
                                 int32_t direction, bvc_stream_codec **out);
int  bvc_stream_codec_set_target(bvc_stream_codec *st, int32_t slot, float target);
int  bvc_stream_codec_sizes(bvc_stream_codec *st, int32_t **d_sizes);
int  bvc_stream_codec_bits(bvc_stream_codec *st, float **d_bits);

/* BVRNNCodecModel.encode (bvrnn_codec_model.py:44-62): scale, log-mel, bits/frame =
 * bits_per_frame for every (b,t), zero initial state, BVRNN.encode.  d_wav (B,L) -> d_codes. */
int bvc_encode(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale,
               float bits_per_frame, float *d_codes, void *d_ws, size_t ws_bytes, void *stream);

/* BVRNNCodecModel.decode (bvrnn_codec_model.py:64-71): zero state, BVRNN.decode, vocoder, /scale. */
int bvc_decode(const bvc_model *m, const float *d_codes, int32_t B, int64_t T, int64_t length,
               float out_scale_div, float *d_wav, void *d_ws, size_t ws_bytes, void *stream);

/* bvc_decode with lost frames concealed from the prior: zero state, bvc_bvrnn_decode_conceal with bits_per_frame for every generated
 * frame (ignored when var_bit = 0), vocoder, / out_scale_div.  d_codes_out (B,T,z_dim) optional: the filled codes.  BVC_EMISSING without
 * the prior.* tensors. */
int bvc_decode_conceal(const bvc_model *m, const float *d_codes, const uint8_t *d_present, float bits_per_frame, int32_t B, int64_t T,
                       int64_t length, float out_scale_div, float *d_wav, float *d_codes_out, void *d_ws, size_t ws_bytes,
                       void *stream);

/* Entropy-coded wire format (new: the reference has no bit stream).  pack / pack_vbr and the session packets spend one stored bit per
 * active code bit; here a bit costs about -log2 of the probability the model's prior net (bvrnn.py:68-73) gives it at the decoder's own
 * state.  Lossless, for storage and reliable transport: a backward-adaptive coder loses synchronism for the rest of a row when a
 * segment is lost, so lossy transport keeps the fixed wire and concealment.  The rate gain on trained checkpoints has NOT been
 * measured (the shipped checkpoints are stubs); a prior that does not predict the bits makes the stream LONGER than the fixed wire.
 * A stream is decodable by the same build on the same architecture only (format tag 0x01, kept in documentation, not in the stream).
 *
 * The coder: a binary range coder with carry propagation, 32-bit range, 33-bit low, 16-bit probabilities
 * q = clamp(rint(p * 65536), 1, 65535) = P(bit = 1), p the float32 probability (round-half-even).  Encoder state low = 0 (64-bit),
 * range = 0xFFFFFFFF, cache = 0, cache_size = 1.  One bit b under q: bound = (range >> 16) * (65536 - q); b == 0: range = bound, else
 * low += bound, range -= bound; while range < 2^24: shift_low(), range <<= 8.  shift_low: if (uint32)low < 0xFF000000 or low >> 32:
 * emit cache + carry, then cache_size - 1 bytes 0xFF + carry (carry = low >> 32), cache = (low >> 24) & 0xFF, cache_size = 0; always
 * cache_size += 1, low = (low & 0x00FFFFFF) << 8.  End of a segment: five times shift_low; the first emitted byte (always 0) is not
 * stored, trailing zero bytes are stripped, a segment without a coded bit has 0 bytes.  Decoder: range = 0xFFFFFFFF, code = the first
 * four stored bytes big-endian, a read at or beyond the segment's size yields 0; one bit: code < bound: 0, range = bound, else 1,
 * code -= bound, range -= bound; while range < 2^24: code = (code << 8) | next byte, range <<= 8.
 * What is coded: for frame t of a row the positions n = 0 .. z_dim - 1 in order that carry a bit, bits[b, t] > n (every position on a
 * fixed-rate model); the coded bit is code > 0.5; a position without a bit is not coded and decodes to 0.5.  Segment s of a row holds
 * the frames [s S, min((s + 1) S, T)), S = min(segment, T), and starts a fresh coder.  d_data (B, nseg, stride) uint8, d_sizes
 * (B, nseg) int32, nseg = ceil(T / S); bytes from size to stride are zero.  bvc_entropy_stride(z_dim, segment) =
 * 2 S z_dim + S / 16 + 8 is a stride no segment exceeds; with a smaller one a segment that does not fit gets size -1 and nothing is
 * written beyond the stride.  The decoder takes a size outside [0, stride] as 0 bytes (BVC_EINVAL before anything is launched where
 * d_sizes is pinned host memory).
 *
 * bvc_entropy_encode / bvc_entropy_decode: the coder on a GIVEN probability tensor d_prob (B,T,z_dim), no model involved; d_bits (B,T)
 * or NULL for bits_per_frame everywhere.  z_dim a multiple of 4.
 * bvc_bvrnn_entropy_pack: bvc_bvrnn_decode_conceal with every frame present - on whatever schedule the model takes - and the encoder
 * behind it, under that call's prior probabilities.  d_bits (B,T) required when var_bit = 1.  Optional: d_h0, d_hT, d_prior (B,T,z_dim).
 * bvc_bvrnn_entropy_unpack: the receive program.  The decoder must know prior(h_t) before it knows z_t, and h_{t+1} depends on z_t, so
 * the range decoder runs INSIDE the frame: the concealing call's step - prior.{0,2,4} and the code epilogue by the same kernel,
 * parameters and order of summation, so p_t is the sender's number - then one node that decodes z_t from the stream, then phi_z, dec,
 * the hop and the GRU unchanged.  By induction it visits the sender's states and returns its mel and h_T bit for bit.  Always the
 * launch-per-layer schedule (cached hipGraph replay, or eager).  d_codes (B,T,z_dim), d_hT, d_prior optional; d_mel (B,T,num_mels).
 * bvc_decode_entropy: zero state, the receive program, the generator, / out_scale_div - as bvc_decode_conceal is composed.
 * Workspace of the three model calls: bvc_entropy_workspace_bytes(m, B, T) - NOT bvc_workspace_bytes.  BVC_EMISSING without prior.*;
 * BVC_EINVAL: segment < 1, stride < 0, z_dim > 3 h_dim, a null argument.  Not supported: streaming sessions, mixed-length batches,
 * bit counts carried in the stream. */
int64_t bvc_entropy_stride(int32_t z_dim, int64_t segment);
size_t bvc_entropy_workspace_bytes(const bvc_model *m, int32_t B, int64_t T);
int bvc_entropy_encode(const float *d_codes, const float *d_prob, const float *d_bits, float bits_per_frame, int32_t B, int64_t T,
                       int32_t z_dim, int64_t segment, uint8_t *d_data, int64_t stride, int32_t *d_sizes, void *stream);
int bvc_entropy_decode(const uint8_t *d_data, int64_t stride, const int32_t *d_sizes, const float *d_prob, const float *d_bits,
                       float bits_per_frame, int32_t B, int64_t T, int32_t z_dim, int64_t segment, float *d_codes, void *stream);
int bvc_bvrnn_entropy_pack(const bvc_model *m, const float *d_codes, const float *d_bits, const float *d_h0, int32_t B, int64_t T,
                           int64_t segment, uint8_t *d_data, int64_t stride, int32_t *d_sizes, float *d_hT, float *d_prior, void *d_ws,
                           size_t ws_bytes, void *stream);
int bvc_bvrnn_entropy_unpack(const bvc_model *m, const uint8_t *d_data, int64_t stride, const int32_t *d_sizes, const float *d_bits,
                             const float *d_h0, int32_t B, int64_t T, int64_t segment, float *d_codes, float *d_mel, float *d_hT,
                             float *d_prior, void *d_ws, size_t ws_bytes, void *stream);
int bvc_decode_entropy(const bvc_model *m, const uint8_t *d_data, int64_t stride, const int32_t *d_sizes, float bits_per_frame, int32_t B,
                       int64_t T, int64_t segment, int64_t length, float out_scale_div, float *d_wav, float *d_codes, void *d_ws,
                       size_t ws_bytes, void *stream);

/* Mixed-length batches: utterances of their own lengths (and bitrates) in ONE call, each coded exactly as it would be alone.
 * d_lengths / d_frames are DEVICE int64 arrays (B).  The library cannot look at them without synchronising, so validating them is
 * the CALLER's job; the kernels only clamp (lengths into [0, L], frames into [0, T]), and a row too short for the reflect padding
 * (bvc_num_frames(length) <= 0) yields all-0.5 codes / an all-zero waveform without touching memory out of bounds.  Workspace:
 * bvc_workspace_bytes(m, B, T) as for bvc_encode / bvc_decode.  Asynchronous, no allocation, capturable, like every compute entry point.
 *
 * Encode: row b of d_wav (B, L) holds d_lengths[b] <= L valid samples (the rest of the row is never read); d_bits (B) bits per frame
 * per utterance, or NULL for bits_per_frame everywhere.  d_codes (B, T, z_dim), T = bvc_num_frames(L); frames t >= T_b =
 * bvc_num_frames(d_lengths[b]) of row b are 0.5.  Row b == bvc_encode of that utterance alone (its T_b frames), bit for bit. */
int bvc_encode_ragged(const bvc_model *m, const float *d_wav, const int64_t *d_lengths, int32_t B, int64_t L, float scale,
                      const float *d_bits, float bits_per_frame, float *d_codes, void *d_ws, size_t ws_bytes, void *stream);
/* Decode: d_frames (B) valid frames per row (<= T), d_lengths (B) samples wanted per row; d_wav (B, n_max),
 * 0 < n_max <= bvc_vocoder_length(m, T).  Row b == bvc_decode(codes[b, :frames_b], length_b) in its first
 * min(length_b, bvc_vocoder_length(frames_b)) samples (clamped to n_max) and 0 after them; code frames behind frames_b are never
 * read into those samples. */
int bvc_decode_ragged(const bvc_model *m, const float *d_codes, const int64_t *d_frames, int32_t B, int64_t T,
                      const int64_t *d_lengths, int64_t n_max, float out_scale_div, float *d_wav, void *d_ws, size_t ws_bytes,
                      void *stream);

/* BVRNNCodecModel.forward (bvrnn_codec_model.py:73-76: decode(encode(x, bitrate), x.shape[1])) WITHOUT the second recurrence.  The
 * encoder's frame loop already runs the decoder on every frame (bvrnn.py:198-204) from exactly the states BVRNN.decode would visit
 * again from the same codes (bvrnn.py:222-227), so its outputs are handed to the vocoder directly: one recurrence launch instead of two,
 * no all-frame phi_z GEMMs.  Not a replacement for bvc_encode + bvc_decode (which stay the reference's two operators and the path the
 * benchmark's headline times): the two differ in the ORDER in which dec.0 and the GRU's input gates sum their halves, i.e. by rounding
 * (tests: waveform within 1e-5 RMS of bvc_decode(bvc_encode(x)), codes identical).  d_codes (B, T, z_dim) optional. */
int bvc_forward(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale, float bits_per_frame, int64_t length,
                float out_scale_div, float *d_codes, float *d_wav_out, void *d_ws, size_t ws_bytes, void *stream);

/* Closed-loop variable-rate encoding (new: the reference takes the bits of every frame from its caller, bvrnn.py:163-194).  The caller
 * states a distortion target per frame and a ladder of bit counts; the encoder, which runs the decoder on every frame anyway
 * (bvrnn.py:198-204), spends the fewest bits of the ladder that meet the target.  Per utterance b and frame t at state h_t:
 *   p = sigmoid(enc([phi_x(norm(y_t)), h_t])), z = round(p)                                  - the plain encoder;
 *   for every rung k: z^k = z on positions < n_k and 0.5 behind them, d^k = dec([phi_z(z^k), h_t]),
 *                     D_k = mean_j |d^k_j - y_{t,j}| over the num_mels bands, in float32, summed in an order that depends on the row alone;
 *   k* = the first k with D_k <= target[b, t], the last rung if there is none (so a NaN or -inf target gives the last rung, +inf rung 0);
 *   codes[b, t] = z^{k*}, bits[b, t] = n_{k*}, and the recurrence goes on with rung k*: h_{t+1} = GRU([phi_x(norm(d^{k*})), phi_z(z^{k*})], h_t).
 * With K = 1 the result is bvc_bvrnn_encode at n_0 bits, bit for bit.  The codes need no side information: bvc_bvrnn_decode, the
 * concealing decoder and the streaming receiver take them unchanged.
 *   d_mel (B,T,num_mels); d_target (B,T) in the units of the natural-log mel; h_ladder: K HOST int32, 1 <= K <= 8, each in [0, z_dim],
 *   strictly ascending; d_h0 (B,h_dim) or NULL.  Outputs: d_codes (B,T,z_dim), d_bits (B,T) float; optional (may be NULL) d_all_h
 *   (B,T,h_dim) the state BEFORE each frame, d_hT (B,h_dim), d_prob (B,T,z_dim), d_dist (B,T,K) = D, d_dec (B,T,num_mels) = d^{k*}.
 * The candidates run as K * B rows of the recurrent-layer kernels, on the launch-per-layer schedule whatever the `recurrence` option says
 * and on the unfolded layer list (`encode_fold` does not apply: dec.6 must exist to be measured).  Workspace: bvc_vbr_workspace_bytes(m, B,
 * T, K) - NOT bvc_workspace_bytes.  BVC_EINVAL: a fixed-rate model (var_bit = 0: there is no mask), a bad ladder, a short workspace.
 * bvc_encode_vbr: the front-end of bvc_encode (scale, log-mel, zero state) followed by the above; d_target (B, bvc_num_frames(L)). */
size_t bvc_vbr_workspace_bytes(const bvc_model *m, int32_t B, int64_t T, int32_t K);
int bvc_bvrnn_encode_vbr(const bvc_model *m, const float *d_mel, const float *d_target, const int32_t *h_ladder, int32_t K,
                         const float *d_h0, int32_t B, int64_t T, float *d_codes, float *d_bits, float *d_all_h, float *d_hT,
                         float *d_prob, float *d_dist, float *d_dec, void *d_ws, size_t ws_bytes, void *stream);
int bvc_encode_vbr(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale, const float *d_target,
                   const int32_t *h_ladder, int32_t K, float *d_codes, float *d_bits, void *d_ws, size_t ws_bytes, void *stream);
/* The same with a hard cap on the rate: an integer token bucket per row inside the selection.  Units are q8 (1/256 bit) in int32;
 * rate_q8 >= 0 and burst_q8 >= 0 are the same for every row, the state is tok[b].  For row b at frame t, once k_target - the choice of
 * the rule above - is known:
 *   1. tok = min(burst_q8, tok + rate_q8)
 *   2. a = the largest k with ladder[k] * 256 <= tok, 0 if there is none
 *   3. k* = min(k_target, a): codes, bits, the decoded mel and the recurrence all go on with k*
 *   4. tok = max(0, tok - ladder[k*] * 256)
 * Integers only, so the result is exact on every schedule.  If ladder[0] * 256 <= rate_q8, every window of L consecutive frames of a row
 * holds 256 * sum(bits) <= burst_q8 + L * rate_q8.  A target of -inf spends whatever the bucket allows (a rate target).
 *   d_tok0 (B) int32 or NULL = a full bucket (burst_q8) in every row; d_tokT (B) or NULL: the state behind the last frame.  A sequence
 *   cut into calls carries d_tokT into d_tok0 as it carries d_hT into d_h0; the result does not depend on where the cut is.
 * BVC_EINVAL: a negative parameter; burst_q8 < ladder[0] * 256 (such a bucket never holds rung 0).  bvc_encode_vbr_capped: behind the
 * front-end of bvc_encode_vbr, zero state, full buckets.  The uncapped entries run none of this. */
int bvc_bvrnn_encode_vbr_capped(const bvc_model *m, const float *d_mel, const float *d_target, const int32_t *h_ladder, int32_t K,
                                const float *d_h0, int32_t B, int64_t T, float *d_codes, float *d_bits, float *d_all_h, float *d_hT,
                                float *d_prob, float *d_dist, float *d_dec, void *d_ws, size_t ws_bytes, void *stream, int32_t rate_q8,
                                int32_t burst_q8, const int32_t *d_tok0, int32_t *d_tokT);
int bvc_encode_vbr_capped(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale, const float *d_target,
                          const int32_t *h_ladder, int32_t K, float *d_codes, float *d_bits, void *d_ws, size_t ws_bytes, void *stream,
                          int32_t rate_q8, int32_t burst_q8);

/* Pre-processing of the reference's example.py:15-17.
 * bvc_resample_poly: y = upfirdn(h, x, up, down)[n_pre_remove : n_pre_remove + n_out] with zero padding, i.e.
 * scipy.signal.resample_poly once the caller has designed / padded the filter h (float64, device memory) as
 * scipy does; d_x (B, L_in) -> d_y (B, n_out).  bvc_peak_normalize: x[b,:] /= max|x[b,:]| in place. */
int bvc_resample_poly(const float *d_x, int32_t B, int64_t L_in, const double *d_h, int32_t ntaps, int32_t up,
                      int32_t down, int64_t n_pre_remove, float *d_y, int64_t n_out, void *stream);
int bvc_peak_normalize(float *d_x, int32_t B, int64_t L, void *stream);

/* Streaming resampler (not in the reference): bvc_resample_poly a chunk at a time, for B rows with lives of their own - what puts a
 * streaming session in front of a client that speaks 8 .. 48 kHz, float32 or s16.  The filter is the one scipy.signal.resample_poly(x,
 * rate_out, rate_in) designs (up = rate_out / gcd, down = rate_in / gcd, Kaiser beta 5, n_pre_remove = the lag in output samples), and
 * one output is the sum bvc_resample_poly forms, term for term in float64.  So the outputs a row has got are a BIT-EXACT PREFIX of
 * bvc_resample_poly on that row's own signal, however it was cut into chunks:
 *  - output m needs the inputs up to floor((m + n_pre_remove) * down / up); after N inputs exactly
 *    E(N) = max(0, ceil(N * up / down) - n_pre_remove) outputs are complete (bvc_resampler_count: host arithmetic, 64 bit, no device);
 *  - a push of n_in inputs gives a row E(N + n_in) - E(N) outputs; a flush gives the rest up to ceil(N * up / down), with zeros for the
 *    inputs behind the end - what bvc_resample_poly's clamp at the signal's end amounts to.
 * State per row, in device memory owned by the object: the last `history` = ceil(ntaps / up) inputs and the input count.
 *  - create: every row idle.  max_in: the longest chunk; history + max_in float32 must fit 64 KiB (BVC_EINVAL otherwise).  fmt_in /
 *    fmt_out: BVC_PCM_F32, or BVC_PCM_S16 (in: x / 32768, exact; out: clamp(rintf(y * 32768), -32768, 32767) of the float32 value the
 *    f32 path would have stored, NaN gives 0 - the s16 result is a function of the f32 result).  fmt_out | BVC_PCM_DELAYED: the row's
 *    output stream is zeros(n_pre_remove) followed by the outputs, of which ceil(N * up / down) samples are complete after N inputs - a
 *    chunk with n_in * up % down == 0 then gives EVERY running row exactly n_in * up / down samples, the first chunk included (a
 *    session's input side: a fixed hop in, a fixed hop out); a flush gives the last n_pre_remove.  The library designs the filter
 *    itself, in float64, restating numpy's firwin / kaiser / i0 operation for operation (bvc_resampler_taps gives the taps, no device);
 *    the two agree to the last bit where exp, sin and sqrt of the two C libraries do.  A caller whose reference is a numpy design hands
 *    its own taps in (set_taps: host memory, the design's ntaps, before the first push; it copies synchronously).
 *  - open (reset + run), close (idle) and end are host bookkeeping between two pushes: they neither launch, allocate nor synchronise.
 *    The next push carries them to the device on its own stream, ahead of its own work (one small launch per 64 changed rows).  open:
 *    history zero, N = 0, and the row's first sample is sample offset_in_next_push of the next chunk (a stream that starts inside a
 *    chunk).  end: the row's stream ends with the first n_valid_in_next_push samples of the next chunk; what lies behind them is not
 *    read, the row takes nothing after that push and waits for its flush (or close, or open).
 *  - push: the same n_in for every row; row b reads d_x + b * x_row_stride (elements of the input format) and writes its outputs from
 *    d_y + b * y_row_stride + y_offset (elements of the output format) on; the positions behind them up to ceil(n_in * up / down) are
 *    written as zeros, so a row of d_y holds at least that many behind y_offset.  An idle (or ended) row's input is NEVER read - NaN,
 *    Inf, uninitialised memory there reach nothing - and its output is zeros.  One launch over all rows; no allocation, no
 *    synchronisation; capturable.  h_counts (B, host, may be NULL): the rows' output counts, from E by arithmetic.
 *  - flush: the rest of a running or ended row, *count <= n_pre_remove samples, to d_y_row (one launch); the row is idle afterwards.
 *  - lag: n_pre_remove and history of a pair of rates (no device).
 * BVC_EINVAL with the object untouched: a row out of range, open on a running row, end on one that is not, flush of an idle one,
 * n_in > max_in, a row that starts or ends behind n_in, rates <= 0.  One in-flight push per object. */
typedef struct bvc_resampler bvc_resampler;
enum { BVC_PCM_F32 = 0, BVC_PCM_S16 = 1, BVC_PCM_DELAYED = 16 };
int  bvc_resampler_create(int32_t B, int32_t rate_in, int32_t rate_out, int32_t max_in, int32_t fmt_in, int32_t fmt_out,
                          bvc_resampler **out);
void bvc_resampler_destroy(bvc_resampler *r);
int  bvc_resampler_set_taps(bvc_resampler *r, const double *h_taps, int32_t ntaps);
int  bvc_resampler_open(bvc_resampler *r, int32_t row, int32_t offset_in_next_push);
int  bvc_resampler_close(bvc_resampler *r, int32_t row);
int  bvc_resampler_end(bvc_resampler *r, int32_t row, int32_t n_valid_in_next_push);
int  bvc_resampler_push(bvc_resampler *r, const void *d_x, int64_t x_row_stride, int32_t n_in, void *d_y, int64_t y_row_stride,
                        int64_t y_offset, int32_t *h_counts, void *stream);
int  bvc_resampler_flush(bvc_resampler *r, int32_t row, void *d_y_row, int32_t *count, void *stream);
int64_t bvc_resampler_count(int32_t rate_in, int32_t rate_out, int64_t n_inputs);
int  bvc_resampler_lag(int32_t rate_in, int32_t rate_out, int32_t *n_pre_remove, int32_t *history);
int  bvc_resampler_taps(int32_t rate_in, int32_t rate_out, double *h_taps, int32_t capacity);   /* returns ntaps; writes if capacity >= ntaps */

/* The multi-rate streaming resampler: the same object with a RATE PER ROW, for a session whose clients speak different rates.  Every row
 * is converted between ITS rate and one fixed rate, all rows in the one launch of a push; a row at rate r gets, bit for bit, what a
 * single-rate object between r and fixed_rate gives it (both kernels form an output in the same function), so the prefix contract above
 * holds per row.
 *  - create_multi: n_rates = 1 .. 8 distinct positive rates; direction 0 converts rates[i] -> fixed_rate (a session's input side), 1
 *    fixed_rate -> rates[i] (its output side).  max_in[i]: the longest chunk of a row at rates[i], on the input side; history_i +
 *    max_in[i] float32 must fit 64 KiB for every i.  Formats and BVC_PCM_DELAYED as above, for the whole object.  Entry i has its own
 *    filter, designed as above; set_taps_rate hands in a caller's taps for entry rate_index (the design's ntaps of THAT pair of rates).
 *    All arguments are checked before a device is touched (BVC_EINVAL).
 *  - open_rate: open with the row's rate, an index into rates[].  The rate is the row's from there until the row is idle again (close,
 *    or flush) and opened anew - at any rate: its history is reset over the widest entry's length.  close, end, flush and destroy are
 *    the calls above and work on either kind of object; end's bound is the row's own max_in, flush uses the row's own filter.
 *  - push_multi: n_in[i] (n_rates entries, 0 allowed) is the chunk length of the rows at rates[i]: rows of one rate share it, different
 *    rates need not.  Row b reads n_in[its rate] samples from d_x + b * x_row_stride (x_row_stride >= the largest n_in[i]) and writes
 *    its outputs from d_y + b * y_row_stride + y_offset on; the positions behind them are written as zeros up to the call's largest
 *    ceil(n_in[i] * up_i / down_i), for EVERY row (y_row_stride >= that), so an idle row's block is zeros and its input is never read.
 *    One launch over all rows, its LDS the largest history_i + n_in[i] of the call; no allocation, no synchronisation.  h_counts: each
 *    row's count by its own rate's E.
 * BVC_EINVAL with the object untouched, and a message that names the other call: open, push or set_taps on a multi-rate object;
 * open_rate, push_multi or set_taps_rate on a single-rate one.  Also: n_rates outside 1 .. 8, a rate <= 0 or listed twice, a
 * rate_index out of range, n_in[i] > max_in[i], a running row that starts or ends behind n_in of its rate. */
int  bvc_resampler_create_multi(int32_t B, int32_t n_rates, const int32_t *rates, int32_t fixed_rate, int32_t direction,
                                const int32_t *max_in, int32_t fmt_in, int32_t fmt_out, bvc_resampler **out);
int  bvc_resampler_set_taps_rate(bvc_resampler *r, int32_t rate_index, const double *h_taps, int32_t ntaps);
int  bvc_resampler_open_rate(bvc_resampler *r, int32_t row, int32_t rate_index, int32_t offset_in_next_push);
int  bvc_resampler_push_multi(bvc_resampler *r, const void *d_x, int64_t x_row_stride, const int32_t *n_in, void *d_y,
                              int64_t y_row_stride, int64_t y_offset, int32_t *h_counts, void *stream);

/* Wire format for the codes (new: the reference keeps them as float32 {0,1,0.5}, bvrnn.py:191-196, and
 * defines no bit stream).  A frame is ceil(nbits/8) bytes, bit i at byte i/8 position i%8 (LSB first);
 * nbits = min(z_dim, bits per frame) active bits are kept, the masked ones (0.5) are re-created on
 * unpack.  d_bytes (B, T, ceil(nbits/8)) uint8; unpack(pack(codes)) == codes for codes from encode(). */
int bvc_pack_codes(const float *d_codes, int32_t B, int64_t T, int32_t z_dim, int32_t nbits, uint8_t *d_bytes,
                   void *stream);
int bvc_unpack_codes(const uint8_t *d_bytes, int32_t B, int64_t T, int32_t z_dim, int32_t nbits, float *d_codes,
                     void *stream);

/* The wire format with a bit count PER FRAME (the codes of bvc_bvrnn_encode_vbr).  A frame has a fixed stride of 1 + ceil(z_dim/8)
 * bytes: byte 0 is the frame's bit count n, the next ceil(n/8) bytes are its bits in bvc_pack_codes order, the rest of the stride is
 * zero.  d_bytes (B, T, 1 + ceil(z_dim/8)); d_bits (B,T) float; d_sizes (B,T) int32 (may be NULL) = 1 + ceil(n/8), the bytes worth
 * sending.  Unpack reads a header above z_dim as z_dim - no read leaves the frame's stride, whatever the bytes hold -, writes 0.5 at
 * positions >= n and n to d_bits (may be NULL).  z_dim <= 255. */
int bvc_pack_codes_vbr(const float *d_codes, const float *d_bits, int32_t B, int64_t T, int32_t z_dim, uint8_t *d_bytes,
                       int32_t *d_sizes, void *stream);
int bvc_unpack_codes_vbr(const uint8_t *d_bytes, int32_t B, int64_t T, int32_t z_dim, float *d_codes, float *d_bits, void *stream);

/* ---- building blocks exported for the parity tests (tests/ only; same kernels the path uses) */
/* The select kernel of bvc_bvrnn_encode_vbr alone, on one frame (allocates, synchronises): d_melhat (K, B, num_mels) the decoded mel of
 * every rung, d_y (B, num_mels), d_tau (B), h_ladder K host int32 -> d_dist (B, K) = D, d_choice (B) int32 = k*, d_bits (B) = n_{k*}. */
int bvc_test_vbr_select(const float *d_melhat, const float *d_y, const float *d_tau, const int32_t *h_ladder, int32_t K, int32_t B,
                        int32_t num_mels, float *d_dist, int32_t *d_choice, float *d_bits, void *stream);
/* ... under the cap of bvc_bvrnn_encode_vbr_capped: d_tok (B) int32, the buckets in front of the frame in, behind it out */
int bvc_test_vbr_select_capped(const float *d_melhat, const float *d_y, const float *d_tau, const int32_t *h_ladder, int32_t K, int32_t B,
                               int32_t num_mels, float *d_dist, int32_t *d_choice, float *d_bits, void *stream, int32_t rate_q8,
                               int32_t burst_q8, int32_t *d_tok);
/* y[M,N] = act(x[M,K] @ w[N,K]^T + bias), act: 0 none, 1 ELU.  Recurrent-step kernel. */
int bvc_test_linear(const float *d_x, const float *d_w, const float *d_bias, int32_t M, int32_t N,
                    int32_t K, int32_t act, float *d_y, void *stream);
/* same contract through the batched (all-frames) GEMM kernel */
int bvc_test_linear_batched(const float *d_x, const float *d_w, const float *d_bias, int32_t M,
                            int32_t N, int32_t K, int32_t act, float *d_y, void *stream);
/* The weight-gradient kernel of the backward pass alone (allocates, synchronises): d_dw (N, K) = d_dy (M, N)^T d_x (M, K), the sum over
 * the M rows of the outer products, overwritten.  All three natural, dense, 16-byte aligned, in device memory; f32 in, f32 accumulated
 * (v_mfma_f32_16x16x4_f32), no atomics: the order of summation is a function of (M, N, K) alone, two calls give
 * the same bits.  out_cut[2] (may be NULL) = the chunks the rows were cut into, and the rows of a chunk.  BVC_EINVAL, before anything
 * touches a device, unless M >= 1 and N and K are multiples of 16, and for a missing or misaligned matrix. */
int bvc_test_weight_grad(const float *d_dy, const float *d_x, int32_t M, int32_t N, int32_t K, float *d_dw, int64_t *out_cut,
                         void *stream);
/* Which instantiation of the recurrent-step kernel a launch of M rows takes (host arithmetic only: needs no GPU).  epi: 0 linear, 1 ELU,
 * 2 code, 3 mel, 4 GRU, 5 GRU with side-branch parts, 6 sigmoid; gate_il: gate-interleaved weights (GRU only); mtw: the row tiles of 16
 * per workgroup asked for (BVC_MTW); latency: BVC_LATENCY=1.  out[2] = the kernel (0 SK_GRU, 1 SK_GRU_IL, 2 SK_GRU_IL2, 3 SK_GRU_PART,
 * 4 SK_LIN, 5 SK_LIN_LATENCY, 6 SK_LIN2, 7 SK_LIN4) and the row tiles per workgroup it runs. */
int bvc_test_skinny_pick(int32_t M, int32_t epi, int32_t gate_il, int32_t mtw, int32_t latency, int32_t *out);
/* Host-side launches of the recurrent-step kernel in this process so far: out[16], [k] the one-frame launches of kernel k (numbered as
 * above), [8 + k] its multi-frame launches (several frames in one grid).  A launch captured into a graph counts once, at capture. */
int bvc_test_skinny_counts(int64_t *out);
/* bvc_test_linear with the caller's row tiles per workgroup (mtw; clamped by the row count as in the path) over `frames` independent
 * frames: d_x (frames, M, K) -> d_y (frames, M, N); frames > 1 is ONE multi-frame launch.  BVC_EINVAL, with nothing launched, if N or K
 * is no multiple of 16 or frames < 1. */
int bvc_test_linear_tiles(const float *d_x, const float *d_w, const float *d_bias, int32_t M, int32_t N, int32_t K, int32_t act,
                          int32_t mtw, int32_t frames, float *d_y, void *stream);
/* How a launch is cut into tiles (host arithmetic only: needs no GPU).  kind 0: the batched GEMM over rows x (column_blocks *
 * 128) outputs; 1: the offline AMP pair of the C = 64 stage over rows output rows x column_blocks batch items with ks taps.  mode 0: the planned cut, 1: the cut of before the plan (BVC_TILE_CUT=legacy), >= 16: that tile height forced (height 0
 * comes back if it is not compiled), -1: what the last launch of that kind in this process used (other arguments ignored).
 * out[6] = tile height, row blocks of that height (GEMM: of the first launch; AMP: tiles per batch item), height of the tail
 * launch's tiles (0: one launch), tiles, rounds, model cost in hundredths of a row. */
int bvc_test_tile_plan(int32_t kind, int64_t rows, int32_t column_blocks, int32_t ks, int32_t mode, int64_t *out);
/* ONE launch of the front-end kernel (synchronises) with the caller's frame count T and left padding instead of the model's:
 * d_wav (B, L) -> d_mel (B, T, num_mels); frame t of a row reads its samples 256 t - pad_left + [0, 1024), reflected once at 0 and
 * at the row's end.  d_lengths (B) int64 or NULL: the valid samples per row, as in bvc_encode_ragged (the row reflects at its own
 * end, its frames behind that hold the log floor).  Refused with BVC_EINVAL, in this order and before the model is looked at:
 * pad_left outside [0, 768]; T < 1; a T whose last frame reads a reflected sample outside [0, L); with d_lengths, a T above the
 * frames of a full row. */
int bvc_test_stft_logmel(const bvc_model *m, const float *d_wav, const int64_t *d_lengths, int32_t B, int64_t L, int64_t T,
                         int32_t pad_left, float scale, float *d_mel, void *stream);
/* dump of one vocoder intermediate, channels-last: which = 0 conv_pre, 1+2i up_i, 2+2i stage_i.
 * Runs the vocoder up to that point.  d_out (B, len, C); returns len*C via *out_numel_per_batch. */
int bvc_test_vocoder_tap(const bvc_model *m, const float *d_mel, int32_t B, int64_t T, int32_t which,
                         float *d_out, int64_t *out_numel_per_batch, void *d_ws, size_t ws_bytes,
                         void *stream);

/* ONE layer of the generator on a caller-supplied input, through the launchers and the packed weights the path uses (no arithmetic of
 * its own).  d_x (B, L, Cin) channels-last in device memory; d_out channels-last; L >= 1.  kind:
 *   0 conv_pre: (B, L, num_mels) -> (B, L, upsample_initial_channel);
 *   1 upsampler `stage`: (B, L, Cin) -> (B, (L + 1) * rate, C);
 *   2 AMP pair (stage, block, iteration): out = x + conv2(S2(conv1_dil(S1(x)))), (B, L, C) -> (B, L, C).  epi 1: that; 2: d_acc + that;
 *     3: (d_acc + that) / number of AMP blocks.  d_acc (B, L, C) is the running sum and may be d_out itself, as in the path.
 *     window != 0: the buffer is a streaming window - row 0 is global time t_origin, rows before row_begin are history and only rows
 *     [row_begin, L) of d_out are written; S2 rows before global time 0 are zero.  window == 0: the offline sweep.
 *   3 activation_post -> conv_post -> tanh -> / div: (B, L, C) -> (B, min(length, L)).
 * Arguments a kind does not use are ignored.  out_info[5] (may be NULL) = output rows per item, output channels, and for kind 2 what
 * the launch was cut into: tiles, workgroups launched (fewer than tiles: a persistent kernel walks over several tiles per workgroup),
 * output rows per tile. */
int bvc_test_vocoder_layer(const bvc_model *m, int32_t kind, int32_t stage, int32_t block, int32_t iteration,
                           const float *d_x, int32_t B, int64_t L, float *d_out, int32_t epi, const float *d_acc,
                           int32_t window, int64_t row_begin, int64_t t_origin, int64_t length, float div,
                           int64_t *out_info, void *stream);

/* ONE symmetric AMP pair (stage, block, iteration) in a look-ahead window, as the incremental generator launches it: d_x (B, L_in, C)
 * is a window whose row 0 is global time t_origin and whose L_in rows are all the pair may read (rows from L_in on read as zeros,
 * and S2 is zero behind it as before global time 0); only rows [row_begin, row_end) of d_out (B, L_in, C) are written, 0 <= row_begin
 * <= row_end <= L_in.  Mid-stream row_end = L_in - (ks-1)(d+1)/2; row_end = L_in is the end of the signal.  epi, d_acc and out_info
 * as in bvc_test_vocoder_layer.  BVC_EINVAL unless the stage is symmetric. */
int bvc_test_amp_pair_window(const bvc_model *m, int32_t stage, int32_t block, int32_t iteration, const float *d_x, int32_t B,
                             int64_t L_in, float *d_out, int32_t epi, const float *d_acc, int64_t row_begin, int64_t row_end,
                             int64_t t_origin, int64_t *out_info, void *stream);

/* y[i] = SnakeBeta(x[i]) = x + sin(x*exp(alpha))^2 / (exp(beta) + 1e-9)  (activations.py:107-120), through the
 * device routines of the generator kernels (their sin^2 is a hand-written range reduction, not ocml's sinf). */
int bvc_test_snakebeta(const float *d_x, int64_t n, float alpha, float beta, float *d_y, void *stream);

/* ---- bench instrumentation: in-situ hipEvent timing of one kernel family inside the real schedule.
 * kind: 1 recurrent linear layer, 2 GRU cell, 3 vocoder conv, 4 batched phi_x GEMM, 5 STFT/mel,
 * 6 conv_post.  Every `sample_every`-th launch of that family is bracketed by an event pair on its
 * own stream until `max_samples` pairs are used; bvc_probe_end synchronises the device and returns
 * the mean / min elapsed microseconds.  Not thread-safe; off by default. */
int bvc_probe_begin(int32_t kind, int32_t sample_every, int32_t max_samples);
int bvc_probe_end(double *mean_us, double *min_us, int32_t *n_samples);
/* The recurrent BVRNN kernels are replayed from a hipGraph, where event pairs cannot be inserted:
 * with bvc_kprobe_enable(1) every workgroup of those kernels stamps wall_clock64() (100 MHz) at its
 * start and end into a device buffer; bvc_kprobe_read returns the mean/min kernel duration
 * (first workgroup start -> last workgroup end) over all frames of the LAST bvrnn encode/decode call
 * for the step-kernel indices [node_lo, node_hi).  Encode step: 0 enc.0, 1 enc.2, 2 enc.4(+sigmoid/
 * round/mask), 3-5 phi_z, 6-9 dec, 10-12 phi_x, 13 GRU.  Decode step: 0-3 dec, 4-6 phi_x, 7 GRU. */
int bvc_kprobe_enable(int32_t on);
int bvc_kprobe_read(int32_t node_lo, int32_t node_hi, double *mean_us, double *min_us, int32_t *n_samples);
/* Persistent recurrence only: one wave (workgroup BVC_PROBE_WG, wave BVC_PROBE_WAVE; default 0 / 0) stamps per layer and frame:
 * 0 layer entered, 1 output published; a library built with -DBVC_FLOW_DIAG=1 also 2 flags seen, 3 products done, 4 reduction
 * barrier passed, 5 layer left.  Mean / min of (stamp `to` - stamp `from`) over the frames of the LAST call for the layers
 * [node_lo, node_hi); from = -1 measures from the stamp 1 of the nearest earlier layer that ran (with the folded hop the program has no dec.6
 * node: its slot stays empty and its row reads 0). */
int bvc_kprobe_read_span(int32_t from, int32_t to, int32_t node_lo, int32_t node_hi, double *mean_us, double *min_us,
                         int32_t *n_samples);

#ifdef __cplusplus
}
#endif
#endif /* BVCODEC_H */
