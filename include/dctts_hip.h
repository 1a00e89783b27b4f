/* dctts_hip.h -- C ABI of the MI355X-native DC-TTS synthesis path (libdctts_hip.so).
 *
 * The reference (Kyubyong/dc_tts) has no FFI / plugin registry; the seam it offers is the Python
 * function surface of networks.py, called from train.py:55,58,64,68,77 and driven by
 * synthesize.py:47-57.  Each entry point below replaces one of those call sites and is what a
 * binding (ctypes / cgo / JNI) would target; the Python host layer dc_tts_amd/networks.py is one
 * such binding and mirrors the reference's names and argument order.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer on the context's GPU unless it says "host";
 *   - tensors are channel-last, contiguous: (B, time, C) float32; ids/indices int32 in,
 *     max_attentions int64 out (tf.argmax default), exactly as the reference graph;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are stream-ordered
 *     and never synchronise the device, except where noted (weight upload; dropping the workspace
 *     cache once it outgrows dctts_set_workspace_limit);
 *   - streams and threads (round 5): any entry point may be called from any stream and any host thread.
 *     Calls of one context that share scratch memory are ORDERED on the device whatever streams they come
 *     from -- TextEnc calls with each other and with decodes, decodes with each other, SSRN calls with each
 *     other (a later call waits for the earlier one's completion event) -- so results never depend on what
 *     else is in flight; calls of DIFFERENT kinds on different streams overlap (SSRN of batch n beside the
 *     decode of batch n + 1).  The host side of a context is serialised by a mutex (enqueue only);
 *   - return value 0 = ok, negative = dctts_status; nothing throws across the ABI;
 *   - only training=False (inference) semantics exist: dropout (modules.py:139,195,245) is identity.
 */
#ifndef DCTTS_HIP_H
#define DCTTS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dctts_ctx dctts_ctx;

typedef enum {
  DCTTS_OK = 0,
  DCTTS_ERR_ARG = -1,       /* bad pointer / shape / mode (the reference would raise from TF) */
  DCTTS_ERR_HIP = -2,       /* a HIP runtime call failed: see dctts_last_error() */
  DCTTS_ERR_WEIGHTS = -3,   /* missing / mis-shaped variable, or weights not finalized */
  DCTTS_ERR_STATE = -4
} dctts_status;

/* hyperparams.py:19,14,29-32,38-39 -- the constants the kernels are specialised on */
typedef struct {
  int vocab_size;   /* len(hp.vocab) = 32 */
  int e;            /* 128 */
  int d;            /* 256 */
  int c;            /* 512 */
  int n_mels;       /* 80 */
  int n_linear;     /* 1 + n_fft/2 = 1025 */
  int max_N;        /* 180 */
  int attention_win_size; /* 3 */
} dctts_config;

/* Lifetime.  One context per (process, GPU); thread-safe per context (see "streams and threads" above). */
int dctts_create(dctts_ctx** out, int device, const dctts_config* cfg);
int dctts_destroy(dctts_ctx* ctx);
const char* dctts_last_error(void);

/* Weights: replaces the implicit tf.get_variable / tf.layers variables restored by name in
 * synthesize.py:32-40.  `name` is the TF variable name, e.g.
 * "Text2Mel/AudioEnc/HC_7/conv1d/kernel"; `data` is a HOST float32 array in TF layout
 * (conv kernel (k,Cin,Cout); conv2d_transpose kernel (1,k,Cout,Cin)).  finalize packs every
 * kernel into MFMA fragment order and uploads (synchronises the device). */
int dctts_weights_set(dctts_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim);
int dctts_weights_finalize(dctts_ctx* ctx);

/* networks.py:14  TextEnc(L) -> (K, V).  L (B,N) int32; K,V (B,N,d). */
int dctts_textenc_fwd(dctts_ctx* ctx, const int32_t* L, int B, int N, float* K, float* V, void* stream);
/* networks.py:73  AudioEnc(S) -> Q.  S (B,T,n_mels); Q (B,T,d).  Causal. */
int dctts_audioenc_fwd(dctts_ctx* ctx, const float* S, int B, int T, float* Q, void* stream);
/* networks.py:126 Attention(Q,K,V,mononotic_attention,prev_max_attentions) -> (R, alignments, max_attentions).
 * Q (B,T,d); K,V (B,N,d); prev_max (B,) int32 (required iff monotonic); R (B,T,2d);
 * alignments (B,N,T) or NULL; max_attentions (B,T) int64 or NULL.  Monotonic mode requires
 * N == max_N (the mask is built from hp.max_N, networks.py:142-143). */
int dctts_attention_fwd(dctts_ctx* ctx, const float* Q, const float* K, const float* V, int B, int T, int N,
                        int monotonic, const int32_t* prev_max, float* R, float* alignments,
                        int64_t* max_attentions, void* stream);
/* networks.py:157 AudioDec(R) -> (logits, Y).  R (B,T,2d); logits,Y (B,T,n_mels). */
int dctts_audiodec_fwd(dctts_ctx* ctx, const float* R, int B, int T, float* logits, float* Y, void* stream);
/* networks.py:214 SSRN(Y) -> (logits, Z).  Y (B,T,n_mels); logits,Z (B,4T,n_linear); logits may be NULL. */
int dctts_ssrn_fwd(dctts_ctx* ctx, const float* Y, int B, int T, float* logits, float* Z, void* stream);

/* synthesize.py:45-54: the autoregressive Text2Mel loop for max_T = T steps, as an incremental
 * decoder that is arithmetically the reference's full-recompute loop (TextEnc once, AudioEnc
 * incrementally, windowed attention + the 85-row AudioDec dependency cone re-evaluated with the
 * current window at every step).  L (B,N) int32, N == max_N.  Y (B,T,n_mels) out;
 * max_attentions (B,T) int64 out or NULL (column j = the value fed back as prev_max at step j+1);
 * alignments (B,N,T) out or NULL = `g.alignments` as the loop's LAST sess.run fetches it (synthesize.py:48,
 * networks.py:153): every time row against the window of step T-1.
 * A decode that fails on the device (see dctts_decode_status) overwrites Y / alignments with NaN and
 * max_attentions with -1 before the call's work on `stream` ends. */
int dctts_text2mel_decode(dctts_ctx* ctx, const int32_t* L, int B, int N, int T, float* Y,
                          int64_t* max_attentions, float* alignments, void* stream);
/* synthesize.py:45-57: decode + one SSRN pass.  Z (B,4T,n_linear) (NaN as well after a failed decode). */
int dctts_synthesize(dctts_ctx* ctx, const int32_t* L, int B, int N, int T, float* Y, float* Z,
                     int64_t* max_attentions, float* alignments, void* stream);

/* Status of the decodes issued so far on this context; call after synchronising their stream.  The default decode form runs two
 * kernels per frame whose workgroups wait for each other inside the launch (bounded waits, about a second at most: a stalled
 * stream must not hang the queue).  When a wait gives up -- the GPU is shared with another process's kernels, or a team of
 * workgroups was not placed on one XCD -- that decode is INVALID: its last kernel overwrites its outputs with NaN / -1 and raises a
 * sticky status word on the device that no later decode clears.  This call returns DCTTS_ERR_STATE once for all decodes that
 * failed since the previous call (the message has the count and the error bits) and clears the word; a failure nobody asked
 * about makes the next decode call on the context fail instead of running.  Time-outs leave the team kernels on (three failed
 * reports in a row switch them off); a misplaced team switches them off for good.  dc_tts_amd.Engine.synchronize() calls this;
 * Engine.text2mel / synthesize(check=True) also repeat a failed decode once in the safe form (dctts_decode_safe_once). */
int dctts_decode_status(dctts_ctx* ctx);

/* The NEXT decode on this context (only that one) runs in the form that cannot time out: one launch per layer, and the two
 * decode streams meet through stream wait / write operations instead of bounded in-kernel waits (~1.5x the frame time).  The
 * persistent settings -- dctts_set_team_kernels, a switch-off by dctts_decode_status -- are left exactly as they were.  This is
 * what a caller does after dctts_decode_status reported a failed decode (the GPU is shared with somebody else's kernels). */
int dctts_decode_safe_once(dctts_ctx* ctx);

/* 1 (default): runs of dependent layers of a decode frame are ONE launch whose workgroups meet inside an XCD's L2
 * (csrc/xgroup_kernel.h, xcone_kernel.h); 0: one launch per layer (no hand-offs between the workgroups of a launch; ~1.3x the frame time). */
int dctts_set_team_kernels(dctts_ctx* ctx, int enable);

/* Decode launch mode: 0 (default) = every launch eager; 1 = the side-stream (bulk) work of each frame is one hipGraph launch,
 * the latency-critical chain launches stay eager.  Measured on MI355X: a graph launch costs ~10 us of start-up on a path that is
 * ~100 us per frame, so the eager form is the faster one and the default. */
int dctts_set_decode_graph(dctts_ctx* ctx, int enable);

/* Decode algorithm form (results agree to fp32 re-association; both are the exact-parity incremental decode):
 * 3 = (default) column-split chain kernels that contract only each layer's centre tap on the caller's stream (older taps arrive as
 *     presums computed on a side stream), AudioDec C_1 / HC_2 cone rows as row operations on cached V.W / Q.W products
 *     (csrc/decode3_kernels.h),
 * 0 = fused full-row kernels on one stream with a device-side frame counter (one workgroup per 32-row block): the simplest form, a
 *     different implementation of the same arithmetic, kept as a cross-check.
 * The forms measured and dropped in rounds 1-2 (two-stream split kernels, one row-split launch per chain piece, persistent highway
 * groups, in-kernel gates) are in the git history up to commit 19f2cbe. */
int dctts_set_decode_mode(dctts_ctx* ctx, int mode);

/* Device memory the context holds for the shapes seen so far (weights + workspaces), bytes. */
size_t dctts_device_bytes(const dctts_ctx* ctx);

/* OPT-IN reduced-cost contraction for the two throughput networks; the default (0) is exact fp32 everywhere and is what every number quoted as the
 * metric is measured with.  mode 1: SSRN's convolutions, mode 2: SSRN's and TextEnc's run on the bf16 matrix pipe from SPLIT operands -- every fp32
 * weight and activation is written as hi + mid (two bf16 terms, round-to-nearest) and a product is accumulated in fp32 as hi.hi + hi.mid + mid.hi
 * (v_mfma_f32_32x32x16_bf16: 16x the fp32 matrix rate, three instructions instead of eight per 16 k); what is dropped is <= 2^-16 of |x||w| per product.
 * Bias, layer-norm, gate, activations and the 1025th column stay fp32; AudioEnc / Attention / AudioDec (the decode, whose arg-max is fed back:
 * synthesize.py:52-54) always run in fp32, so with mode 1 the mel output and the attention trajectory are bit-identical to mode 0.  Call it BEFORE
 * dctts_weights_finalize with the highest level wanted (the weights get a second, bf16 packing); afterwards any level up to that one can be selected per call
 * sequence.  Measured error against the float64 oracle: tests/test_gpu_parity.py::test_split_bf16_*, DESIGN.md section 11. */
int dctts_set_split_bf16(dctts_ctx* ctx, int mode);

/* Which arithmetic the split-bf16 networks run (dctts_set_split_bf16 says WHICH networks; the decode never runs in either).  terms = 2 (default): the form above.
 * terms = 3: every weight and activation is written as hi + mid + lo, three bf16 terms (round-to-nearest-even; lo = bf16(x - hi - mid) from the exact remainder, so the
 * three terms carry all 24 mantissa bits and x = hi + mid + lo exactly), and a product is accumulated in fp32 from SIX matrix instructions, small products first:
 * lo.hi + hi.lo + mid.mid + mid.hi + hi.mid + hi.hi.  Every bf16 x bf16 product is exact in fp32; what is dropped, mid.lo + lo.mid + lo.lo, is <= ~2^-26 of |x||w|
 * per product, below one fp32 accumulate rounding (2^-24), and the accumulator is rounded 6 times per 16 k against 8 in the fp32 form: fp32-grade error at
 * 6 x 32 matrix cycles per 16 k against 8 x 64 (fp32) and 3 x 32 (two terms).  The weights' packing has three fragments per group instead of two, so the value in force
 * at dctts_weights_finalize is the one the context keeps: afterwards a different value is DCTTS_ERR_STATE (the same value is accepted).  Anything but 2 or 3 is
 * DCTTS_ERR_ARG.  Measured error and time: tests/test_gpu_split_bf16_terms.py, DESIGN.md section 11. */
int dctts_set_split_bf16_terms(dctts_ctx* ctx, int terms);

/* The same choice for the TRAINING path (handle of dctts_train.h): which arithmetic its contractions run: every GEMM behind the hc / conv1d / conv1d_transpose forward and backward passes (pre-norm
 * tensors, input gradients, split-K weight gradients) and the attention forward and backward.  terms = 0 (default): v_mfma_f32_32x32x2_f32, exact fp32 products.
 * terms = 3: every element of BOTH operands is written as hi + mid + lo, three bf16 terms that carry all 24 mantissa bits (x = hi + mid + lo exactly), inside the
 * GEMM on its way into LDS, and a product is accumulated in fp32 from SIX v_mfma_f32_32x32x16_bf16 instructions, small products first: lo.hi + hi.lo + mid.mid +
 * mid.hi + hi.mid + hi.hi.  What is dropped (mid.lo + lo.mid + lo.lo) is <= ~2^-26 of |a||b| per product, below one fp32 accumulate rounding: fp32-grade
 * gradients on the bf16 matrix pipe.  The row kernels (layer-norm, gate, softmax, losses, dropout, Adam) are fp32 either way.  Nothing is packed, so the setting may
 * change between any two calls and the tape is unaffected; sums keep their fixed order (bitwise reproducible in either form).  Two differences from the fp32 form: an
 * infinite operand gives NaN (inf - inf in the split) where fp32 gives +-inf, and operands below ~2^-100 lose their low terms to bf16 underflow.  Anything but 0 or 3
 * is DCTTS_ERR_ARG.  Measured error and time: tests/test_gpu_train_split_bf16.py, DESIGN.md section 10, profiles/train_split_bf16.txt. */
struct dctts_train;
int dctts_train_set_split_bf16_terms(struct dctts_train* t, int terms);

/* Workspaces and the decode's device tables are cached per geometry (B, T, N) and only grow: a serving loop that alternates
 * between batch shapes pays an allocation the first time a shape is seen and nothing afterwards (no hipDeviceSynchronize, no
 * hipFree on a shape change).  When the cached workspaces exceed `bytes` (default 96 GiB of the 288 GB) the next call drops
 * all of them behind ONE device synchronisation and starts again. */
int dctts_set_workspace_limit(dctts_ctx* ctx, size_t bytes);

/* Test / measurement hooks (per-layer test entry, calibration copy, kernel timing) are declared in
 * dctts_hip_debug.h: they are not part of the drop-in surface. */

/* ------------------------------------------------------------------------------------------------
 * Vocoder tail: utils.py:67-114 `spectrogram2wav` / `griffin_lim` / `invert_spectrogram`, which
 * synthesize.py:61-64 calls once per utterance on the CPU (librosa + scipy).  Here: a batch at a time on the GPU.
 * It owns no weights, so it is its own handle.  Spectrogram tensors stay frame-major (B, F, 1 + n_fft/2) -- the layout
 * dctts_ssrn_fwd writes (F = 4T) -- not librosa's (1 + n_fft/2, F). */
typedef struct dctts_vocoder dctts_vocoder;

/* hyperparams.py:13-24 + the librosa.effects.trim defaults the reference relies on (utils.py:92) */
typedef struct {
  int n_fft;            /* 2048 (the reference: one frame per 1024-point complex transform, 1025 bins) or 1024 (two adjacent frames per transform,
                         * 513 bins); anything else is DCTTS_ERR_ARG */
  int hop_length;       /* 275 */
  int win_length;       /* 1102 */
  int n_iter;           /* 50 */
  float power;          /* 1.5 */
  float preemphasis;    /* 0.97 */
  float max_db;         /* 100 */
  float ref_db;         /* 20 */
  float trim_top_db;    /* 60 */
  int trim_frame_length;/* 2048 */
  int trim_hop_length;  /* 512 */
} dctts_vocoder_config;

int dctts_vocoder_create(dctts_vocoder** out, int device, const dctts_vocoder_config* cfg);
int dctts_vocoder_destroy(dctts_vocoder* v);
size_t dctts_vocoder_device_bytes(const dctts_vocoder* v);

/* utils.py:67-94 spectrogram2wav for B utterances.  mag (B,F,1+n_fft/2): network output in [0,1] (Z).
 * wav (B, hop_length*(F-1)) float32: de-normalise -> **power -> Griffin-Lim (n_iter) -> de-emphasis, NOT trimmed;
 * bounds (B,2) int32 or NULL: [start, end) of librosa.effects.trim(wav) per utterance (the reference returns
 * wav[start:end]).  Requires hop_length*(F-1) > n_fft/2 (reflect padding; librosa raises below that too). */
int dctts_spectrogram2wav(dctts_vocoder* v, const float* mag, int B, int F, float* wav, int32_t* bounds, void* stream);

/* utils.py:96-106 griffin_lim on magnitudes.  spec (B,F,1+n_fft/2) (already de-normalised, any non-negative values);
 * y (B, hop_length*(F-1)); X_best (B,F,1+n_fft/2,2) interleaved complex64 or NULL = the spectrogram*phase the last
 * iteration produced (needs n_iter >= 1).  n_iter = 0 gives y = istft(spec). */
int dctts_griffin_lim(dctts_vocoder* v, const float* spec, int B, int F, int n_iter, float* y, float* X_best, void* stream);

/* Fast Griffin-Lim (Perraudin, Balazs, Soendergaard 2013) in the form of librosa.griffinlim(momentum=...): with
 * beta = momentum / (1 + momentum) every iteration projects the phase of  t = c - beta * c_prev  instead of that of
 * c = stft(istft(X)), c_prev = 0 in the first.  0 <= momentum < 1, anything else (NaN too) is DCTTS_ERR_ARG; 0, the
 * default, is the reference's loop (utils.py:96-106), bit for bit.  Holds for dctts_spectrogram2wav and
 * dctts_griffin_lim from the next call on.  A non-zero momentum costs one more signal buffer (B, hop_length*(F-1))
 * floats, counted by dctts_vocoder_device_bytes once a call with n_iter >= 2 has used it; X_best != NULL together
 * with it is DCTTS_ERR_ARG.  Results stay bitwise reproducible and independent of the rest of the batch. */
int dctts_vocoder_set_momentum(dctts_vocoder* v, float momentum);

/* The analysis direction: utils.py:18-65 get_spectrograms and the frame reduction of load_spectrograms (:155-164) for a RAGGED batch of waveforms.
 * dctts_vocoder_set_mel_basis: basis_host (n_mels, 1 + n_fft/2) row-major on the HOST, what librosa.filters.mel returns; packed once into a band table
 * (first bin, width) + the non-zero weights and uploaded.  DCTTS_ERR_ARG if a row's non-zeros are not one contiguous run, a band is wider than 96 bins
 * (the kernel sums a band with 16 lanes in at most 6 rounds) or n_mels is not a multiple of 4.  The call waits for the device (set-up, not per batch).
 *
 * dctts_wav2spectrograms: wav (B, Lmax) float32, zero past each length; lengths (B) int32; both on the DEVICE, as are all outputs.  trim != 0:
 * librosa.effects.trim per utterance (cfg.trim_*), then y'[n] = y[n] - preemphasis y[n-1], |stft|, mel projection, 20 log10(max(1e-5, .)), normalisation to
 * [1e-8, 1].  With Fmax = 1 + Lmax / hop_length and Fpad = Fmax rounded up to a multiple of r (>= 1):
 *   mag (B, Fpad, 1 + n_fft/2) or NULL;   mel (B, Fpad / r, n_mels) or NULL: frames 0, r, 2r, ... (needs the basis: DCTTS_ERR_STATE without it);
 *   bounds (B, 2) or NULL: the trimmed [start, end) (trim = 0: (0, length));
 *   n_frames (B) or NULL: F_b = 1 + (end - start) / hop_length, the frames before padding -- rows at or past it are 0.0, which is load_spectrograms' zero
 *   padding; 0 = nothing left (a clip of zeros; the numpy path keeps such a clip whole and returns floor values); -1 = the untrimmed or the trimmed signal
 *   has at most n_fft/2 samples, where reflect padding is undefined (all its rows are 0.0).  Neither touches the other utterances.
 * Stream-ordered, no host synchronisation (workspaces grow with the largest call); results are bitwise reproducible and do not depend on the rest of the
 * batch.  Lmax must exceed n_fft/2.  The trim decision is taken in fp32, the transform too (audio.py: float64).
 * Cross-talk at n_fft = 1024: frames 2p and 2p + 1 of an utterance share one fp32 transform, so a frame's rounding error is relative to the LOUDER of the
 * two, not to itself (about 1e-7 of the louder frame's peak).  At ordinary levels that is below the normalisation floor of 1e-5; a frame 60 dB or more
 * under its neighbour (the first frame of an onset) carries it visibly in its weakest bins.  n_fft = 2048 has one frame per transform and no such term. */
int dctts_vocoder_set_mel_basis(dctts_vocoder* v, const float* basis_host, int n_mels);
int dctts_wav2spectrograms(dctts_vocoder* v, const float* wav, const int32_t* lengths, int B, int Lmax, int trim, int r,
                           float* mel, float* mag, int32_t* n_frames, int32_t* bounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCTTS_HIP_H */
