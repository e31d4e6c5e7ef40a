/*
 * bsrnn_hip.h -- C ABI of the MI355X-native BSRNN separation path (libbsrnn_hip.so).
 *
 * This is the drop-in boundary: plain C, plain pointers and sizes, no torch / C++ types.
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repo phhusson/SpeechSeparation).  Host bindings (ctypes, the LADSPA plugin,
 * or a libtorch/pybind stub in the reference itself) bind exactly these symbols; see
 * INTEGRATION.md for the reference-side stubs.
 *
 * Conventions
 *   - all tensors are contiguous float32;
 *   - "dev" pointers are device (HIP) pointers on the context's device, "host" pointers are
 *     ordinary host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls enqueue work
 *     and return without synchronising unless stated otherwise;
 *   - return value 0 = success, otherwise a BSRNN_E* code; bsrnn_last_error() gives text;
 *   - nothing here ever falls back to a CPU implementation.
 *
 * Concurrency contract
 *   - ONE call at a time per context.  A context owns one workspace (activations of the call in flight) and one weight
 *     arena; every compute entry point, bsrnn_commit_params and the stream calls of its bsrnn_stream objects count as
 *     calls on it.  A call that arrives from a second host thread while another is inside the library is refused with
 *     BSRNN_ESTATE (it never races).  Use one context per host thread for concurrent work; contexts share nothing.
 *   - Calls enqueue on the caller's HIP stream.  Consecutive calls on the SAME stream are ordered by the stream.  A call
 *     on a DIFFERENT stream than the previous call first waits, on the host, for that previous stream to drain (the two
 *     would otherwise overlap on the workspace): correct, but it serialises - keep a context on one stream.
 *   - A larger call may regrow the workspace and bsrnn_commit_params rebuilds the arena; both wait for the device first,
 *     and bsrnn_stream objects notice (a generation counter) and re-capture their hipGraph at their next step.
 *   - bsrnn_destroy with bsrnn_stream objects still alive only retires the context (further calls: BSRNN_ESTATE); the
 *     memory is released when the last of its streams is destroyed.
 *   - C = rows of dim 0 (utterance-channels), T / L = STFT frames, F2 = 2050 interleaved
 *     re/im columns, K = number of bands including the zero-width band, H = 64.
 */
#ifndef BSRNN_HIP_H
#define BSRNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared in this header are exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BSRNN_ABI_VERSION 2      /* 2: range policy (bsrnn_set_range_policy), training entry points, bsrnn_forward_chunk refuses aliased state */

#define BSRNN_OK          0
#define BSRNN_EARG        1   /* bad argument / shape */
#define BSRNN_ESTATE      2   /* call out of order (e.g. compute before commit) */
#define BSRNN_EHIP        3   /* HIP runtime error */
#define BSRNN_EIO         4   /* weight file problem */
#define BSRNN_ENOKEY      5   /* unknown parameter key */
#define BSRNN_ERANGE      6   /* an activation left the range of the split-precision mode (|a| > 65504), see below */

typedef struct bsrnn_ctx bsrnn_ctx;
typedef struct bsrnn_stream bsrnn_stream;

int         bsrnn_abi_version(void);
const char* bsrnn_last_error(void);
/* How the matrix products are evaluated, e.g. "gemm=fp16x2 lstm=fp16x2" (measurement / logging only).
 * Inputs, outputs, state and accumulation are float32 in every mode; the modes differ in which matrix pipe
 * carries the products: "f32" = v_mfma_f32_*_f32 (exact fp32 fma chains), "fp16x2" = fp32 operands
 * split into 2 fp16 pieces and multiplied on the 16-bit matrix cores with fp32 accumulation
 * (error at the level of fp32 rounding noise).  Selected once per process by the environment
 * variables BSRNN_GEMM (f32 | fp16x2 | fp16) and BSRNN_LSTM (f32 | fp16x2); default fp16x2 for both.
 * BSRNN_GEMM=fp16 is the one REDUCED-precision mode (plain fp16 operands in the Linear layers, one MFMA term,
 * fp32 accumulation: ~1e-3 of the output range); it exists for the "16-bit compute" benchmark configuration.
 * Range: the fp16x2 mode represents operands up to |a| = 65504 (spectra of audio in [-1, 1] stay below 1024).  A larger
 * finite activation cannot be represented; the kernels notice (a host-visible guard word).  What happens then is the
 * context's RANGE POLICY (bsrnn_set_range_policy):
 *   - BSRNN_RANGE_EXACT (default): every model entry point (bsrnn_forward, _forward_chunk, _forward_recurrent, _dual_path,
 *     _separate, _stream_step, _evaluate) waits for its own kernels before it returns, looks at the guard and, if it is set,
 *     runs the same call again on the library's exact-fp32 kernels (fp32 weights are always resident; no range limit) from
 *     the same inputs / the same starting state: rc 0 always comes with correct numbers, as from the reference.  The price
 *     is one stream synchronisation per call.
 *   - BSRNN_RANGE_DEFERRED: the entry points return without waiting (launch pipelines, the benchmark loop).  A violation is
 *     reported late: the NEXT call on the context, bsrnn_sync or bsrnn_stream_get_state fails with BSRNN_ERANGE, once, and
 *     the results of the call that caused it are invalid (not-a-number or nonsense, never silently plausible saturated
 *     values: nothing is clamped).  The caller repeats the work under the default policy.
 *   bsrnn_stream_step_host and bsrnn_evaluate always behave as under BSRNN_RANGE_EXACT (they wait for their kernels anyway).
 * NaN / Inf inputs are not range errors: they come out as NaN, as they do from the reference. */
const char* bsrnn_compute_mode(void);

/* ---- construction -------------------------------------------------------------------
 * Replaces `BSRNN()` (bsrnn.py:328-376).  `widths` are band widths in bins, in order,
 * including the trailing zero-width band (generate_bandsplits()[0], bsrnn.py:247-326);
 * sum(widths) must be 1025.  The band table is data: pass a different one for the
 * 41-band variant.  `device` is the HIP device ordinal, or -1 for a HOST-ONLY context: parameter inventory,
 * bsrnn_set_param / bsrnn_get_param and bsrnn_load_weights_file (as a validator) work without a GPU, every compute
 * entry point returns BSRNN_ESTATE (tools/convert_weights.py, CPU tests). */
int  bsrnn_create(int device, const int32_t* widths, int32_t n_bands, bsrnn_ctx** out);
void bsrnn_destroy(bsrnn_ctx* ctx);
int  bsrnn_n_bands(const bsrnn_ctx* ctx);
int  bsrnn_device(const bsrnn_ctx* ctx);
/* Range policy of the split-precision modes (see bsrnn_compute_mode above); default BSRNN_RANGE_EXACT. */
#define BSRNN_RANGE_DEFERRED 0
#define BSRNN_RANGE_EXACT    1
int  bsrnn_set_range_policy(bsrnn_ctx* ctx, int32_t policy);
int  bsrnn_get_range_policy(const bsrnn_ctx* ctx);
/* 1 when the committed context runs the per-band MLP chains (bsrnn.py:404-415, :420-443) as fused launches (one workgroup =
 * one band's five Linear layers, intermediates in LDS; the default), 0 when it runs one grouped launch per layer: the
 * exact-fp32 mode, BSRNN_MLP=layers (A/B), or a band table with a band too wide for the fused kernel's LDS image
 * (more than 768 columns).  The same fp16x2 products either way; a band whose chain runs the 32 x 32 x 16 geometry without the ragged
 * split (bsrnn_chain_geometry) gives results bit-identical to the per-layer flow, the 16 x 16 x 32 geometries and the ragged split sum
 * in another order and agree with it at fp32 rounding level. */
int  bsrnn_mlp_fused(const bsrnn_ctx* ctx);
/* Geometry of the fused MLP chain of one band of the committed context (measurement / test support).  chain: 0 = bandFCs_pre + bandFCs
 * (bsrnn.py:404-415), 1 = bandFCs_back + bandFCs_back_post (bsrnn.py:420-443); band: 0 .. K-1.  out[6]:
 *   out[0] frame rows per workgroup; out[1] MFMA shape, 32 (32 x 32 x 16) or 16 (16 x 16 x 32); out[2] RT, row tiles per wave group
 *   (of 32 rows in the 32 shape, of 16 in the 16 shape); out[3] NW, waves per group (8 / NW groups); out[4] bit l set when the last
 *   feature tile of layer l is split over the k-steps of all eight waves (the ragged split); out[5] 1 when the 16 shape zeroes the
 *   k-units of its LDS image that a layer's K loop reads but no layer output covers (a layer width N % 32 != 0; always at 64 rows).
 * A zero-width band: all six 0 (no matrix work in either chain).  A context that runs the per-layer flow (bsrnn_mlp_fused() == 0):
 * all six -1 for every band.  BSRNN_EARG for a bad chain or band, BSRNN_ESTATE on a host-only or uncommitted context. */
int  bsrnn_chain_geometry(const bsrnn_ctx* ctx, int32_t chain, int32_t band, int32_t out[6]);
/* How this context runs the dual path of large calls (bsrnn.py:352-356, the four recurrent blocks): 1 = overlapped - the second band
 * block is launched beside the first (causal) time-axis launch and the mask MLPs beside the second, on an auxiliary stream of the
 * context, each workgroup waiting for the frames of its own rows (results are bit-identical to 0); 0 = one launch after the other
 * (environment BSRNN_OVERLAP=0); 2 = switched off for good after a consumer's bounded wait expired once (that call was run again launch
 * after launch before it returned; under the 'deferred' range policy it is reported by the next call instead).  Calls of fewer than
 * 32 frames or 8 rows x 12 bands never overlap.  Measurement / test support. */
int  bsrnn_overlap_state(const bsrnn_ctx* ctx);
/* Measurement / debugging: copy the first `nfloats` floats of one of the context's internal activation buffers of the LAST call to the
 * host (synchronises the device).  which: 0 = Z0, 1 = Z1 (the dual-path tensor's two buffers, [rows*frames][K][64]), 2 = HB1 (the
 * band blocks' fc shares, [rows*frames][K][2][64]), 3 = P, 4 = Yf (band-padded rows of LDP floats). */
int  bsrnn_debug_peek(bsrnn_ctx* ctx, int32_t which, float* host_out, int64_t nfloats);
/* Process-wide counts of what the library has done that does not belong on a real-time thread: which = 0 device / pinned / stream
 * allocations, 1 stream captures begun, 2 graph instantiations, 3 graph launches.  A bsrnn_stream does all of the first three in
 * bsrnn_stream_create (as the reference's plugin does in its constructor, speech-ladspa-onnx.cpp:55-120); its step calls leave them
 * unchanged (tests/test_gpu_entrypoints.py drives the LADSPA plugin's run() and checks).  which = 4 counts work instead: the frame rows
 * (rows x frames, summed over the segments) bsrnn_separate_long_ragged / bsrnn_evaluate_long_ragged have handed to the model - below R * Tmax when rows retire.
 * Any other value: -1. */
long long bsrnn_debug_counter(int32_t which);

/* ---- parameters ---------------------------------------------------------------------
 * Replaces `load_state_dict` (infer.py:19, infer-streaming.py:46): parameters are named
 * by the reference's state_dict keys and given as host float32
 * in torch layout (Linear weight [out,in]).  bsrnn_commit_params() folds/packs/uploads
 * and must be called after the last bsrnn_set_param() and before any compute call. */
int  bsrnn_param_count(const bsrnn_ctx* ctx);
int  bsrnn_param_info(const bsrnn_ctx* ctx, int32_t index, const char** key,
                      int64_t* dim0, int64_t* dim1, int32_t* ndim);
int  bsrnn_set_param(bsrnn_ctx* ctx, const char* key, const float* host_data, int64_t numel);
int  bsrnn_get_param(const bsrnn_ctx* ctx, const char* key, float* host_out, int64_t numel);
int  bsrnn_commit_params(bsrnn_ctx* ctx);
/* Flat weight file (speechseparation_amd/weights.py) -- replaces the ONNX file that
 * speech-ladspa-onnx.cpp:73 opens.  Does set_param for every tensor, then commit.  Every tensor must carry a key of
 * the inventory and exactly its rank and dimensions (BSRNN_ENOKEY / BSRNN_EIO otherwise; sizes are never taken from
 * the file, and nothing throws across this boundary). */
int  bsrnn_load_weights_file(bsrnn_ctx* ctx, const char* path);

/* I/O signature of the one-frame model, as the reference's exported ONNX file declares it (infer-streaming.py:74
 * `torch.onnx.export(..., (x, state))`; read back by the plugin, speech-ladspa-onnx.cpp:82-111, which sizes its state
 * buffers from the shape of the input named "state.0"): index 0 "x.0" [C, 2050] and 1 "state.0" [4, 2, C*K, 64] are
 * inputs, 2 "y.0" [C, 2050] and 3 "new_state.0" [4, 2, C*K, 64] outputs.  Hosts written against that session API can
 * size and name their tensors from here instead of from a model file; C is the caller's row count (2 in the plugin). */
int  bsrnn_io_count(void);
int  bsrnn_io_info(const bsrnn_ctx* ctx, int32_t index, int32_t C, const char** name, int32_t* is_input,
                   int64_t dims[4], int32_t* ndim);

/* ---- model entry points ---------------------------------------------------------------
 * Aliasing (all model entry points): under BSRNN_RANGE_EXACT a call that left the fp16 range is run again from the same inputs,
 * after its first run may already have written its outputs.  So an output buffer must not share any byte with an input the re-run
 * reads (a range overlap, not only an equal pointer): such a call returns BSRNN_EARG, naming the re-run.  Each entry point states
 * which pairs that concerns; under BSRNN_RANGE_DEFERRED there is no re-run and the buffers may alias as before.
 * bsrnn_forward            = BSRNN.forward            (bsrnn.py:385-443)
 *     x_dev [C, 2050, T] -> y_dev [C, 2050, T]   (y = x * mask; x is not modified unless y or mask
 *     overlaps it).  y and mask MAY overlap x under either policy (in place): the re-run starts from the library's own copy
 *     of x, made before anything is written.
 * bsrnn_forward_recurrent  = BSRNN.forward_recurrent  (bsrnn.py:445-510)
 *     x_dev [C, 2050], state_in_dev [4, 2, C*K, 64] -> y_dev [C, 2050], state_out_dev (same
 *     shape; under BSRNN_RANGE_EXACT neither state_out_dev nor y_dev may overlap state_in_dev - BSRNN_EARG otherwise: a call
 *     that left the fp16 range is run again from state_in_dev -; they may alias it under BSRNN_RANGE_DEFERRED; y may overlap x
 *     as in bsrnn_forward.  The same holds for bsrnn_forward_chunk).  State slabs: 0/1 = h/c of lstms.1, 2/3 = h/c of
 *     lstms.3; dim 1 = LSTM layer; dim 2 = c*K + k.
 * bsrnn_forward_chunk      = L consecutive forward_recurrent steps in one call (BASELINE.json
 *     config 3): x_dev [C, 2050, L], state carried causally; L = 1 equals forward_recurrent.
 * mask_dev (optional, may be NULL): receives the mask [C, 2050, T] (bsrnn.py:425-432). */
int  bsrnn_forward(bsrnn_ctx* ctx, const float* x_dev, float* y_dev, float* mask_dev,
                   int32_t C, int32_t T, void* stream);
int  bsrnn_forward_recurrent(bsrnn_ctx* ctx, const float* x_dev, const float* state_in_dev,
                             float* y_dev, float* state_out_dev, int32_t C, void* stream);
int  bsrnn_forward_chunk(bsrnn_ctx* ctx, const float* x_dev, const float* state_in_dev,
                         float* y_dev, float* state_out_dev, int32_t C, int32_t L, void* stream);

/* `self.lstms(z)` alone (bsrnn.py:352-356, :417): z_dev [C, T, K, 64] -> z_out_dev.  state
 * pointers may be NULL (zero initial state, final state discarded).  Under BSRNN_RANGE_EXACT neither z_out_dev nor state_out_dev
 * may overlap z_dev or state_in_dev (BSRNN_EARG: the re-run reads both again); under BSRNN_RANGE_DEFERRED they may. */
int  bsrnn_dual_path(bsrnn_ctx* ctx, const float* z_dev, float* z_out_dev,
                     const float* state_in_dev, float* state_out_dev,
                     int32_t C, int32_t T, void* stream);

/* ---- training step, part 1: the recurrent layers ------------------------------------------
 * The reference trains with torch.autograd (train.py:97-115: `loss.backward()`, `optimizer.step()`); a replacement has to
 * provide the backward pass itself.  These two calls are one `nn.LSTM` layer of NormRNNResidual (bsrnn.py:66-72) with
 * `ndir` directions (2 = bidirectional: direction 1 uses torch's `_reverse` weights and runs the sequence backwards) over
 * N sequences of L steps, zero initial state, exact fp32:
 *   the band-axis BLSTM is N = C*T, L = K, ndir = 2 (bsrnn.py:144-150), the time-axis LSTM N = C*K, L = T, ndir = 1 with the
 *   rows gathered as in bsrnn.py:110-113.
 * All pointers are device memory.  Weights in torch layout: w_ih [ndir][256][IN] (IN = 64 | 128), w_hh [ndir][256][64],
 * gate order i,f,g,o; bias [ndir][256] = b_ih + b_hh.
 *   forward : x [N][L][IN] -> h [N][L][ndir*64]; gates [N][L][ndir][256] (after sigmoid / tanh) and cells [N][L][ndir][64]
 *             are what backward reads.
 *   backward: dh [N][L][ndir*64] = gradient of the loss w.r.t. h  ->  dx [N][L][IN] (NULL: not wanted), dw_ih, dw_hh in the
 *             weights' layouts, db [ndir][256] (= the gradient of b_ih and of b_hh).  Gradients are overwritten, not
 *             accumulated; sums run in a fixed order (bit-reproducible).  Workspace: a grow-only buffer of the context. */
int  bsrnn_lstm_train_forward(bsrnn_ctx* ctx, const float* x_dev, const float* w_ih_dev, const float* w_hh_dev,
                              const float* bias_dev, float* h_dev, float* gates_dev, float* cells_dev,
                              int32_t N, int32_t L, int32_t IN, int32_t ndir, void* stream);
int  bsrnn_lstm_train_backward(bsrnn_ctx* ctx, const float* x_dev, const float* h_dev, const float* gates_dev,
                               const float* cells_dev, const float* dh_dev, const float* w_ih_dev, const float* w_hh_dev,
                               float* dx_dev, float* dw_ih_dev, float* dw_hh_dev, float* db_dev,
                               int32_t N, int32_t L, int32_t IN, int32_t ndir, void* stream);

/* nn.Linear (+ LeakyReLU(0.01) when leaky != 0) of the per-band MLPs and of fc / fc_in (bsrnn.py:333-376, :69, :74) for the
 * training step: y = act(x W^T + b), x [M, K] with row stride ldx (a band is a column block of a wider row), W [N, K] torch
 * layout, y [M, N] with row stride ldy.  Backward: from dy (row stride lddy; and y when leaky) -> dx [M, K] row stride lddx
 * (NULL: not wanted), dw [N, K], db [N]; overwritten, bit-reproducible.  All device pointers, exact fp32. */
int  bsrnn_linear_train_forward(bsrnn_ctx* ctx, const float* x_dev, int32_t ldx, const float* w_dev, const float* b_dev,
                                float* y_dev, int32_t ldy, int32_t M, int32_t K, int32_t N, int32_t leaky, void* stream);
int  bsrnn_linear_train_backward(bsrnn_ctx* ctx, const float* x_dev, int32_t ldx, const float* w_dev, const float* y_dev,
                                 int32_t ldy, const float* dy_dev, int32_t lddy, float* dx_dev, int32_t lddx,
                                 float* dw_dev, float* db_dev, int32_t M, int32_t K, int32_t N, int32_t leaky, void* stream);

/* The same for n layers that share the row count M - the same Linear layer of all bands (bsrnn.py:406-411, :423-425 loop over
 * the bands) - in grouped launches: host arrays [n] of device pointers / leading dimensions / K / N.  dx_dev[i] may be NULL. */
int  bsrnn_linear_group_train_forward(bsrnn_ctx* ctx, int32_t n, const float* const* x_dev, const int32_t* ldx,
                                      const float* const* w_dev, const float* const* b_dev, float* const* y_dev,
                                      const int32_t* ldy, const int32_t* K, const int32_t* N, int32_t M, int32_t leaky, void* stream);
int  bsrnn_linear_group_train_backward(bsrnn_ctx* ctx, int32_t n, const float* const* x_dev, const int32_t* ldx,
                                       const float* const* w_dev, const float* const* y_dev, const int32_t* ldy,
                                       const float* const* dy_dev, const int32_t* lddy, float* const* dx_dev, const int32_t* lddx,
                                       float* const* dw_dev, float* const* db_dev, const int32_t* K, const int32_t* N,
                                       int32_t M, int32_t leaky, void* stream);

/* Row chunks of the weight-gradient reductions of the calls above (measurement / test support): C [N1][N2] = A^T B over M rows
 * (dw_ih: N1 = 256, N2 = IN; dw_hh: N1 = 256, N2 = 64; Linear dw and db: N1 = N, N2 = K, M rows per direction or layer) runs as
 * out[0] chunks of out[1] rows (the last one may be shorter) whose partial products are then added in a fixed order.  A function
 * of the shape only; no context or device needed.  BSRNN_EARG for M outside [1, 2^30], N1 or N2 outside [1, 65536], or a null out. */
int  bsrnn_train_reduction_layout(int32_t M, int32_t N1, int32_t N2, int32_t out[2]);

/* The critic's layers: nn.Conv1d(I, O, kernel 16, stride 3) (+ LeakyReLU(0.01) when leaky != 0) of the reference's Discriminator
 * (bsrnn.py:512-536), forward and backward, exact fp32.  x [C][I][T] (T contiguous), W [O][I][16], b [O] in torch's layouts,
 * T_out = (T - 16) / 3 + 1:
 *   forward : y[c][o][t] = act(b[o] + sum_{i, k} W[o][i][k] * x[c][i][3 t + k])                                  -> y [C][O][T_out]
 *   backward: with dp = dy * act'(y) (slope 0.01 where y <= 0; y is only read when leaky):  db[o] = sum_{c, t} dp[c][o][t],
 *             dW[o][i][k] = sum_{c, t} dp[c][o][t] * x[c][i][3 t + k],  dx[c][i][s] = sum over o and the taps k with (s - k) % 3 == 0 and
 *             0 <= (s - k) / 3 < T_out of W[o][i][k] * dp[c][o][(s - k) / 3].  dx [C][I][T] is written for every s < T (zeros where no
 *             window reaches) and may be NULL (not wanted: the product is skipped); dW, db are overwritten, not accumulated.
 * All pointers are dense device memory.  No atomics: the products over (i, k) run in slabs of input channels and the reductions over
 * (c, t) in chunks of frames, both a function of the shape only (bsrnn_critic_conv_layout) and added in a fixed order, so results are
 * bit-reproducible.  Workspace: the grow-only training buffer of the context.
 * BSRNN_EARG for a null context or pointer, C, I or O < 1, T < 16, and a shape at which x, W, y or the partial sums would pass
 * 2^31 - 1 elements; then BSRNN_ESTATE on a host-only context.  Nothing is launched on a refusal. */
int  bsrnn_critic_conv_forward(bsrnn_ctx* ctx, const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev,
                               int32_t C, int32_t I, int32_t T, int32_t O, int32_t leaky, void* stream);
int  bsrnn_critic_conv_backward(bsrnn_ctx* ctx, const float* x_dev, const float* w_dev, const float* y_dev, const float* dy_dev,
                                float* dx_dev, float* dw_dev, float* db_dev, int32_t C, int32_t I, int32_t T, int32_t O,
                                int32_t leaky, void* stream);
/* How the two calls above cut their sums (measurement / test support; no context or device needed): out[0] = T_out; the forward's
 * K = (i, k) runs in out[1] slabs of out[2] input channels (the last may hold fewer), added in slab order before the bias; the
 * reductions of dW / db run in out[3] chunks of out[4] frames of every row (the last may hold fewer), added in chunk order.
 * BSRNN_EARG as above, or for a null out. */
int  bsrnn_critic_conv_layout(int32_t C, int32_t I, int32_t T, int32_t O, int32_t out[5]);

/* The critic's input as the reference forms it (train-discriminator.py:62-68): torch.stft(wave * scale, n_fft = 4096, hop_length = 1024,
 * window = hann_window(4096)) - centred, reflect padding - followed by torch.cat((X.real, X.imag), dim = 1).  wave: R rows of n > 2048
 * samples, wave_stride floats apart; T = 1 + n / 1024 frames; x [R][4098][T], T contiguous: rows 0 .. 2048 hold the real parts of bins
 * 0 .. 2048, rows 2049 .. 4097 the imaginary parts, and rows 2049 and 4097 are exactly zero.  Each sample is multiplied by scale first,
 * then by the window (the order torch rounds in), so the call with scale s equals the call on the fp32 product wave * s with scale 1 bit
 * for bit.  Exact fp32, no atomics, bit-reproducible; a frame's bits do not depend on the rows or frames around it.  wave is only read.
 * Workspace: the grow-only training buffer of the context, at most 128 * 32 * 4098 floats (67 MB) whatever the clip: the call runs in
 * slabs of rows x frames (bsrnn_critic_spectrum_layout).  Its twiddle and window tables (49 KB) are built and uploaded by a context's
 * first call (bsrnn_debug_counter(0) counts it); bsrnn_create allocates nothing for it.
 * BSRNN_EARG for a null context or pointer, R < 1, n <= 2048, wave_stride < n, a scale that is not finite, and R * 4098 * T beyond
 * 2^31 - 1; then BSRNN_ESTATE on a host-only context.  Nothing is launched on a refusal. */
int  bsrnn_critic_spectrum(bsrnn_ctx* ctx, const float* wave_dev, int64_t wave_stride, float* x_dev,
                           int32_t R, int64_t n, float scale, void* stream);
/* How the call above is cut (measurement / test support; no context or device needed): out[0] = T; out[1] = the slabs, each one launch
 * of the transform and one of the transpose; out[2] = frames per slab (rows go in blocks of min(R, 128), a block's frames in slabs of
 * 32 * (128 / rows per block) frames); out[3] = the workspace in floats.  BSRNN_EARG as above, or for a null out. */
int  bsrnn_critic_spectrum_layout(int32_t R, int64_t n, int64_t out[4]);

/* The committed critic: the whole Discriminator (four layers, the mean over time, the mean over the rows, Linear(32, 1), sigmoid) frozen
 * into an object that scores in one call - the critic as a separator's training loop uses it, under no_grad, while its weights stand.
 *   bsrnn_critic_create   an object for a critic of in_channels input channels on ctx.  Allocates, once, everything the object ever owns
 *                         (three blocks, bsrnn_debug_counter(0)): its own fp32 copy of every parameter and the first layer's weights as
 *                         two fp16 pieces in the matrix cores' operand order - out[9] and out[8] bytes of bsrnn_critic_score_layout,
 *                         about 2 x 268 MB at 4098 channels, 2 x 134 MB at 2050.  On a host-only context the object is made without them
 *                         and answers only its argument checks.  It keeps its context alive like a bsrnn_stream; destroy it with
 *                         bsrnn_critic_destroy (NULL is ignored).
 *   bsrnn_critic_commit   a SNAPSHOT of the parameters (torch's layouts: conv_w_dev[l] [O_l][I_l][16], conv_b_dev[l] [O_l] for the widths
 *                         in_channels -> 1024 -> 128 -> 64 -> 32, lin_w_dev [32], lin_b_dev [1]): copied on `stream`, the first layer split
 *                         on the device (a1 = fp16(a), a2 = fp16(2^11 (a - a1))), max |W| recorded.  Synchronous; the caller's arrays may
 *                         change or go afterwards.  May be repeated (the object then follows the new weights).  A first-layer weight beyond
 *                         +-65504 (or NaN) makes the image unusable: that object scores with the exact kernels, always.
 *   bsrnn_critic_score    x [C][in_channels][T] (T >= 601 contiguous frames) -> score_dev[0], and the first layer's output
 *                         y1 [C][1024][(T - 16) / 3 + 1] when y1_dev is not NULL.  x_order 0: the channels in the reference's order (all real
 *                         parts, then all imaginary parts: bsrnn_critic_spectrum's); x_order 1: the separator's interleaved spectrum (re, im,
 *                         re, im, ...), channel i of the critic reading row 2 i for i < in_channels / 2, else row 2 (i - in_channels / 2) + 1 -
 *                         no reorder copy.  The first layer (over 99 % of the work) follows the context's compute mode like the model entry
 *                         points: fp32 in and out, products as two fp16 pieces on the f16 matrix cores with fp32 accumulation (three terms),
 *                         range guard on x.  Under BSRNN_RANGE_EXACT the call waits and, if an |x| passed 65504, runs again on the exact
 *                         kernels (bsrnn_critic_conv_forward's) before returning; under BSRNN_RANGE_DEFERRED it is asynchronous and
 *                         bsrnn_sync / the next model call report BSRNN_ERANGE.  With BSRNN_GEMM=f32 every layer is exact.  Layers 2 - 4
 *                         are always exact.  No atomics: K runs in slabs of input channels (out[4], out[5] of the layout), added in slab
 *                         order; bit-reproducible.  Workspace: the grow-only training buffer of the context (out[6] floats; out[7] when an
 *                         interleaved x goes through the exact kernels, which read a planar copy); nothing else is allocated.
 * BSRNN_EARG, before anything touches the device and also on a host-only context: a null object or pointer (y1_dev may be NULL), C < 1,
 * T < 601, x_order outside {0, 1}, x_order 1 with an odd in_channels, a tensor or workspace beyond 2^31 - 1 elements, score_dev or
 * y1_dev overlapping x (the re-run reads x again) or each other.  Then BSRNN_ESTATE on a host-only context and before the first commit.
 * Nothing is launched on a refusal. */
typedef struct bsrnn_critic bsrnn_critic;
int  bsrnn_critic_create(bsrnn_ctx* ctx, int32_t in_channels, bsrnn_critic** out);
int  bsrnn_critic_commit(bsrnn_critic* critic, const float* const conv_w_dev[4], const float* const conv_b_dev[4],
                         const float* lin_w_dev, const float* lin_b_dev, void* stream);
int  bsrnn_critic_score(bsrnn_critic* critic, const float* x_dev, int32_t C, int32_t T, int32_t x_order,
                        float* score_dev, float* y1_dev, void* stream);
/* Sizes of a score (no context or device needed): out[0..3] = frames behind the four layers; out[4] = K slabs of the fp16x2 first layer,
 * out[5] = input channels per slab (the last may hold fewer); out[6] = workspace in floats, out[7] = with the planar copy; out[8] = bytes
 * of the fp16x2 image, out[9] = bytes of the fp32 snapshot.  BSRNN_EARG as above, or for a null out. */
int  bsrnn_critic_score_layout(int32_t in_channels, int32_t C, int32_t T, int64_t out[10]);
void bsrnn_critic_destroy(bsrnn_critic* critic);

/* The committed critic's gradient: the score and d score / d x in one call - the critic as the adversarial term of a separator's loss
 * uses it.  Opt-in per object; an object without it behaves as above.
 *   bsrnn_critic_enable_grad  allocates, once, the first layer's weights a second time as two fp16 pieces, in the operand order of the
 *                         product over the OUTPUT channels (out[7] bytes of bsrnn_critic_grad_layout, the size of the first image up to
 *                         padding: one more block, bsrnn_debug_counter(0)), and builds it from the snapshot if a commit exists; every later
 *                         bsrnn_critic_commit rebuilds it.  Idempotent.  BSRNN_ESTATE on a host-only context.
 *   bsrnn_critic_score_grad   score_dev[0] = the bits bsrnn_critic_score gives on the same input, and dx_dev [C][in_channels][T], in x's
 *                         own order (x_order 1: the gradient of row r of the interleaved spectrum lies in row r), = gscale * d score / d x;
 *                         gscale_dev points at one float on the device, NULL means 1.  Every position of dx is written (zeros where no
 *                         window reaches).  Back through the sigmoid, Linear(32, 1), the two means and layers 4, 3, 2 on the exact fp32
 *                         kernels of bsrnn_critic_conv_backward - with no dW or db - then the first layer's dx
 *                             G[(i, k)][t] = sum_o W[o][i][k] dp1[c][o][t],   dx[c][i][s] = sum over k = s % 3, s % 3 + 3, ... of G[(i, k)][(s - k) / 3]
 *                         as two fp16 pieces on the f16 matrix cores with fp32 accumulation (three terms).  dp1 is far below fp16's
 *                         range: the pass that forms it records max |dp1| on the device, the product runs on dp1 * 2^e with the largest
 *                         operand in [2^14, 2^15) and its result is multiplied by 2^-e, both exact; a zero maximum gives dx = 0.  The
 *                         call follows the compute mode and the range policy like bsrnn_critic_score: an |x| beyond 65504 or a
 *                         non-finite dp1 raises the guard, and under BSRNN_RANGE_EXACT forward and backward then run again on the exact
 *                         kernels from the snapshot before the call returns; under BSRNN_RANGE_DEFERRED the call is asynchronous and
 *                         bsrnn_sync reports BSRNN_ERANGE.  BSRNN_GEMM=f32 and a first-layer weight beyond +-65504 go to the exact
 *                         kernels directly.  No fp32 atomics, one workgroup per (8 input channels, 369 positions, row) over all 1024
 *                         output channels: no partial sums, bit-reproducible.  Workspace: the context's grow-only training buffer, out[5]
 *                         floats (out[6] when an interleaved x goes through the exact kernels: a planar copy of x and a planar dx).
 *   bsrnn_critic_layer1_dx    the first layer's dx alone, from a given dp_dev [C][1024][(T - 16) / 3 + 1], on the same path (test and
 *                         measurement support).
 * BSRNN_EARG, before anything touches the device and also on a host-only context: a null object or pointer (gscale_dev may be NULL),
 * C < 1, T < 601, x_order outside {0, 1}, x_order 1 with an odd in_channels, a tensor, image, grid or workspace beyond 2^31 - 1 elements,
 * dx_dev overlapping x_dev, score_dev (or dp_dev), score_dev overlapping x_dev.  Then BSRNN_ESTATE on a host-only context, before the
 * first commit and when the gradient is not enabled.  Nothing is launched on a refusal. */
int  bsrnn_critic_enable_grad(bsrnn_critic* critic, void* stream);
int  bsrnn_critic_score_grad(bsrnn_critic* critic, const float* x_dev, int32_t C, int32_t T, int32_t x_order, const float* gscale_dev,
                             float* score_dev, float* dx_dev, void* stream);
int  bsrnn_critic_layer1_dx(bsrnn_critic* critic, const float* dp_dev, int32_t C, int32_t T, int32_t x_order, float* dx_dev, void* stream);
/* Sizes of a gradient call (no context or device needed): out[0] = tiles of input channels, out[1] = tiles of input positions per row,
 * out[2], out[3], out[4] = channels, positions and frames of a tile (8, 369, 128); out[5] = workspace in floats, out[6] = with the exact
 * chain's planar copies; out[7] = bytes of the dx image.  BSRNN_EARG as above, or for a null out. */
int  bsrnn_critic_grad_layout(int32_t in_channels, int32_t C, int32_t T, int64_t out[8]);

/* The committed critic on a padded batch: one score per CLIP of a rectangle x_dev [R][in_channels][Tmax] (either channel order) whose rows
 * belong to clips of different lengths - clip c owns clip_rows_host[c] consecutive rows of frames_host[c] frames each,
 * 601 <= frames[c] <= Tmax, the rows of all clips summing to R.  What lies behind a row's frames is never read.
 *   bsrnn_critic_score_ragged       scores_dev[c] = sigmoid(Linear(mean over the clip's rows of mean over its own frames of layers(x))): what
 *                               bsrnn_critic_score gives for the clip alone up to the order of the first layer's sums, which is that of the
 *                               rectangle (the K slabs of bsrnn_critic_score_layout(in_channels, R, Tmax)) - a function of (in_channels, R,
 *                               Tmax) and the row's own length, never of the other clips; one clip owning all rows at frames = Tmax gives
 *                               bsrnn_critic_score's bits.  The first layer's workgroups whose 128 frames all lie behind a row's
 *                               (frames - 16) / 3 + 1 return at once.  y1_dev, when not NULL, receives the first layer's output
 *                               [R][1024][(Tmax - 16) / 3 + 1], valid below each row's own length (test and measurement support).
 *   bsrnn_critic_score_grad_ragged  the same scores, and dx_dev [R][in_channels][Tmax] = gscale_dev[c] * d score_c / d x for the rows of
 *                               clip c (gscale_dev [n_clips] on the device, NULL means 1), in x's own order; every position is written,
 *                               zeros behind a row's frames.  The scale of the first layer's dx (bsrnn_critic_score_grad) is formed per
 *                               CLIP: a clip with a tiny gradient beside a large one keeps its own precision.
 *   bsrnn_critic_layer1_dx_ragged   the first layer's dx alone from dp_dev [R][1024][(Tmax - 16) / 3 + 1], zeros behind each row's own
 *                               length (test and measurement support).
 * All follow the compute mode and the range policy as bsrnn_critic_score_grad does: an |x| beyond 65504 INSIDE a row's frames or a
 * non-finite dp1 raises the guard, BSRNN_RANGE_EXACT runs the whole call again on the exact kernels, BSRNN_RANGE_DEFERRED stays
 * asynchronous; BSRNN_GEMM=f32 and a hot weight go to the exact kernels directly.  The two tables travel through the context's upload ring,
 * the workspace is the grow-only training buffer (out[10] / out[11] / out[12] floats of the layout): a second call of a shape allocates
 * nothing.  Bit-reproducible; no fp32 atomics.
 * BSRNN_EARG, before anything touches the device and also on a host-only context: a null object or pointer (y1_dev and gscale_dev may be
 * NULL), n_clips < 1, a clip with fewer than 1 row, with fewer than 601 or more than Tmax frames, rows not summing to R, x_order outside
 * {0, 1}, x_order 1 with an odd in_channels, a tensor, image, grid or workspace beyond 2^31 - 1 elements, overlapping buffers.  Then
 * BSRNN_ESTATE on a host-only context, before the first commit and (the two gradient calls) when the gradient is not enabled. */
int  bsrnn_critic_score_ragged(bsrnn_critic* critic, const float* x_dev, int32_t R, int32_t Tmax, const int32_t* frames_host,
                               const int32_t* clip_rows_host, int32_t n_clips, int32_t x_order, float* scores_dev, float* y1_dev, void* stream);
int  bsrnn_critic_score_grad_ragged(bsrnn_critic* critic, const float* x_dev, int32_t R, int32_t Tmax, const int32_t* frames_host,
                                    const int32_t* clip_rows_host, int32_t n_clips, int32_t x_order, const float* gscale_dev,
                                    float* scores_dev, float* dx_dev, void* stream);
int  bsrnn_critic_layer1_dx_ragged(bsrnn_critic* critic, const float* dp_dev, int32_t R, int32_t Tmax, const int32_t* frames_host,
                                   const int32_t* clip_rows_host, int32_t n_clips, int32_t x_order, float* dx_dev, void* stream);
/* The plan of a ragged call (no context or device needed): out[0..3] = frames behind the four layers at Tmax; out[4], out[5] = K slabs of
 * the first layer and input channels per slab; out[6] = frame tiles per row of the first layer's forward, out[7] = the live ones summed over
 * the rows; out[8] = position tiles per row of its dx, out[9] = the live ones summed over the rows; out[10] = workspace of a score in
 * floats, out[11] = of a score with its gradient, out[12] = with the exact chain's planar copies; out[13] = bytes of the two tables.
 * BSRNN_EARG as above, or for a null out. */
int  bsrnn_critic_ragged_layout(int32_t in_channels, int32_t R, int32_t Tmax, const int32_t* frames_host, const int32_t* clip_rows_host,
                                int32_t n_clips, int64_t out[14]);

/* torch.optim.AdamW(model.parameters(), lr, weight_decay) of train.py:50, one tensor per call: p, m (exp_avg), v (exp_avg_sq)
 * updated in place from the gradient g; `step` counts from 1 (bias correction).  n floats each, device pointers.  The betas are
 * double, as torch's: 1 - beta2 and the bias corrections are formed from them in double (from 0.999f, 1 - beta2 is 1.3e-5 off). */
int  bsrnn_adamw_step(bsrnn_ctx* ctx, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n,
                      float lr, double beta1, double beta2, float eps, float weight_decay, int32_t step, void* stream);

/* The same update for many parameter tensors at once (80 per launch, pointers passed in the kernel arguments): host arrays
 * [n_tensors] of device pointers and of element counts. */
int  bsrnn_adamw_step_multi(bsrnn_ctx* ctx, float* const* p_dev, const float* const* g_dev, float* const* m_dev, float* const* v_dev,
                            const int64_t* sizes, int32_t n_tensors, float lr, double beta1, double beta2, float eps,
                            float weight_decay, int32_t step, void* stream);

/* The same with the step count and the learning rate in DEVICE memory: state_dev = {float lr, float bc1, float bc2s, int32 step}
 * (16 bytes; the caller initialises lr and step - the number of steps taken so far -, the call advances step by one in stream
 * order and derives the bias corrections from it on the device).  Nothing that changes from iteration to iteration travels by
 * value, so a whole training iteration (train.py:97-115: forward, backward, this call) can be captured once into a hipGraph and
 * replayed; the learning rate of a schedule is a 4-byte copy into state_dev between replays. */
int  bsrnn_adamw_step_multi_dev(bsrnn_ctx* ctx, float* const* p_dev, const float* const* g_dev, float* const* m_dev, float* const* v_dev,
                                const int64_t* sizes, int32_t n_tensors, float* state_dev, double beta1, double beta2, float eps,
                                float weight_decay, void* stream);

/* ---- the STFT sandwich of the callers --------------------------------------------------
 * bsrnn_stft   = infer.py:29-33 (dup. m_dataset.py:187-190): wave_dev [R, n] ->
 *                x_dev [R, 2050, T], T = 1 + n/1024; periodic Hann 2048, hop 1024,
 *                center/reflect, onesided, re/im interleaved.  n must be > 1024.
 * bsrnn_istft  = infer.py:35-37: y_dev [R, 2050, T] -> wave_out_dev [R, (T-1)*1024].
 * bsrnn_separate = the whole sandwich fused on the device (frame-major internally, no
 *                [C,2050,T] round trips): wave_dev [R, n] -> wave_out_dev [R, (T-1)*1024].  Under
 *                BSRNN_RANGE_EXACT wave_out_dev must not overlap wave_dev (BSRNN_EARG: the re-run reads the waveform again);
 *                under BSRNN_RANGE_DEFERRED it is not checked (row blocks run concurrently: an overlap is still unsafe). */
int  bsrnn_stft(bsrnn_ctx* ctx, const float* wave_dev, float* x_dev, int32_t R, int64_t n, void* stream);
int  bsrnn_istft(bsrnn_ctx* ctx, const float* y_dev, float* wave_out_dev, int32_t R, int32_t T, void* stream);
/* Backward of bsrnn_istft for the training step (the loss of m_dataset.py:211-216 has a waveform term): dwave_dev
 * [R, (T-1)*1024] = gradient w.r.t. the waveform -> dy_dev [R, 2050, T] = gradient w.r.t. the spectrum (the transpose of
 * torch.istft: zero-padded windowed FFT of dwave / envelope, one-sided bins weighted 1, 2, ..., 2, 1 over 2048, no gradient
 * for the imaginary parts of bins 0 and 1024). */
int  bsrnn_istft_backward(bsrnn_ctx* ctx, const float* dwave_dev, float* dy_dev, int32_t R, int32_t T, void* stream);
int  bsrnn_separate(bsrnn_ctx* ctx, const float* wave_dev, float* wave_out_dev, int32_t R, int64_t n, void* stream);
/* bsrnn_separate_ragged = bsrnn_separate for R clips of DIFFERENT lengths in one call (a validation set, a request queue): wave_dev holds R
 * rows wave_stride floats apart, row r holds lens_host[r] samples, 1024 < lens_host[r] <= wave_stride (what lies behind them in the row is
 * never read).  With T_r = 1 + lens[r] / 1024 and Tmax = the largest T_r, wave_out_dev is [R, (Tmax-1)*1024]: row r holds the
 * (lens[r] / 1024) * 1024 samples bsrnn_separate gives for that clip alone (reflect padding at the clip's own end, not at the stride or at
 * Tmax), then zeros to the end of the row.  The model is causal along time, its band-axis blocks see one frame at a time and rows are
 * independent, so only the STFT and the iSTFT know the lengths: frames t >= T_r of a row enter the model as zero spectra and leave it as
 * zeros, whatever an earlier call left in the workspace.
 *   - Equal lengths: with all lengths n and wave_stride = n the samples are bit-identical to bsrnn_separate(R, n) wherever that call runs
 *     as one row block (the same plan, the same arithmetic per frame).  The call always runs as ONE row block: the two concurrent row
 *     blocks of bsrnn_separate for R >= 128 are not reproduced (as in bsrnn_separate_long).
 *   - Unequal lengths: a row agrees with bsrnn_separate of that clip alone to rounding (the kernels are chosen for R x Tmax, not 1 x T_r).
 *   - Cost: the model runs on all R * Tmax frame rows - padding is paid for, so batch clips of similar length (the Python layer's
 *     separate_many does: spec.ragged_buckets).  Memory: a workspace of R * Tmax frame rows.
 *   - lens_host is ordinary host memory and may be reused as soon as the call returns, under either range policy; the lengths (and the
 *     call's task tables) travel in one grow-only block of the context, made at first use and when R or R * Tmax outgrows it
 *     (bsrnn_debug_counter(0)); a call that fits allocates nothing.
 *   - Range policy as bsrnn_separate: under BSRNN_RANGE_EXACT a call that left the fp16 range is run again in exact fp32 from the same
 *     waveform and the same lengths, so wave_out_dev must not overlap the R * wave_stride floats of wave_dev (BSRNN_EARG); under
 *     BSRNN_RANGE_DEFERRED it is not checked.
 * BSRNN_EARG, before any device work (also on a host-only context, in front of its BSRNN_ESTATE): a null ctx, wave_dev, lens_host or
 * wave_out_dev; R < 1; a length <= 1024 or > wave_stride (the text names the row and the value). */
int  bsrnn_separate_ragged(bsrnn_ctx* ctx, const float* wave_dev, int64_t wave_stride, const int64_t* lens_host,
                           float* wave_out_dev, int32_t R, void* stream);

/* ---- long-form separation: bsrnn_separate in segments, bounded memory ---------------------
 * bsrnn_separate's result for a clip of any length from a workspace of one segment.  Shapes as bsrnn_separate: wave [R, n] ->
 * wave_out [R, (T-1)*1024], T = 1 + n/1024, n > 1024.  The T frames are cut into consecutive segments of seg_frames frames (the last
 * one shorter, down to one frame); each segment runs STFT of its frames (reflect padding at the CLIP's ends, never at a segment
 * edge) -> the model on R * L frame rows, planned like bsrnn_forward_chunk, the time-axis LSTM state carried from segment to segment
 * (the first starts from zeros; the model is causal along time) -> iSTFT of the hops the segment completes, the windowed second half
 * of its last frame carried to the next segment.  Same DSP as bsrnn_separate (Hann synthesis window, sum of squared windows, no delay):
 * given the same spectra the samples are bit-identical; the chunked model agrees with the one-shot model to rounding, as
 * bsrnn_forward_chunk does with bsrnn_forward.  seg_frames >= T: the call IS bsrnn_separate (it delegates: bit-identical);
 * seg_frames < 1: BSRNN_EARG.
 * Memory: workspace of R * min(seg_frames, T) frame rows, task tables of at most two row counts (the full segment and the tail), two
 * sets of LSTM state and of synthesis carry; nothing grows with T.  One fixed seg_frames therefore serves clips of every length from
 * one workspace and one or two tables.
 * Range policy per segment, as bsrnn_stream_process: under BSRNN_RANGE_EXACT the call waits after each segment and runs a segment
 * that left the fp16 range again on the exact-fp32 kernels from that segment's untouched state and carry set; under
 * BSRNN_RANGE_DEFERRED no segment waits.  wave_out must not overlap wave under EITHER policy (BSRNN_EARG): the reflected tail of the
 * clip, and every later segment, is read after early hops have been written.  The two concurrent row blocks of bsrnn_separate for
 * R >= 128 are not used here.
 * bsrnn_separate_long_host: the same with both buffers in ordinary host memory, synchronous.  The library stages through two pinned
 * input windows and two pinned output blocks with device mirrors of the same sizes and copies on a stream of its own, so the upload
 * of segment i+1 and the download of segment i-1 run beside the kernels of segment i.  Device memory of the call is O(R * seg_frames),
 * waveform included; the staging is made at first use and reused while R and seg_frames do not grow (a later call of any n allocates
 * nothing: bsrnn_debug_counter(0)).  Same kernels, same order, same cut: bit-identical to bsrnn_separate_long. */
int  bsrnn_separate_long(bsrnn_ctx* ctx, const float* wave_dev, float* wave_out_dev, int32_t R, int64_t n, int32_t seg_frames,
                         void* stream);
int  bsrnn_separate_long_host(bsrnn_ctx* ctx, const float* wave_host, float* wave_out_host, int32_t R, int64_t n,
                              int32_t seg_frames);
/* bsrnn_separate_long_ragged = bsrnn_separate_ragged in segments: R clips of DIFFERENT lengths, each of any length, from a workspace of
 * R * min(seg_frames, Tmax) frame rows.  Arguments and result as bsrnn_separate_ragged: rows wave_stride floats apart, lens_host[r]
 * samples in row r (1024 < lens_host[r] <= wave_stride, nothing behind them is read), wave_out_dev [R, (Tmax-1)*1024] with row r holding
 * the (lens[r] / 1024) * 1024 samples of that clip, then zeros; all of it is written.  The Tmax frames are cut as bsrnn_separate_long cuts
 * them.  Segment i, frames [ta, te), runs on the ALIVE PREFIX of the rows, R_i = 1 + the last row r with T_r > ta: STFT of those rows
 * (reflect padding at each clip's own ends; a row's frames at and behind T_r are zero spectra) -> the model on R_i * (te - ta) frame rows
 * with the time-axis state carried -> iSTFT of the segment's hops over all R rows (zeros where a row has ended).  Rows are never
 * reordered: a row inside the prefix that has already ended is carried as zero frames, so any order gives each clip's result, and
 * LONGEST FIRST is the cheap one - then the model runs on about the real frames, rounded up to a segment per row
 * (bsrnn_debug_counter(4) counts them).  When the prefix shrinks the surviving rows' state and overlap-add tail are packed by one small
 * launch on the caller's stream; nothing is allocated or waited for.
 *   - seg_frames >= Tmax: the call IS bsrnn_separate_ragged (it delegates: bit-identical).  Equal lengths: bit-identical to
 *     bsrnn_separate_long(R, n, seg_frames).  Unequal lengths: a row agrees with bsrnn_separate of that clip alone to rounding.
 *   - Before the first launch: the workspace, the task tables of every distinct R_i * (te - ta) of the call, the two carry sets of
 *     bsrnn_separate_long for R rows; the lengths go up once per call through the pinned mirrors of bsrnn_separate_ragged's block, so
 *     lens_host is the caller's again at return.  A second call that fits allocates nothing (bsrnn_debug_counter(0)).
 *   - Range policy per segment, as bsrnn_separate_long; wave_out_dev must not overlap the R * wave_stride floats of wave_dev under
 *     EITHER policy.
 * BSRNN_EARG, before any device work (also on a host-only context, in front of its BSRNN_ESTATE): a null ctx, wave_dev, lens_host or
 * wave_out_dev; R < 1; seg_frames < 1; a length <= 1024 or > wave_stride (the text names the row and the value); R * min(seg_frames, Tmax)
 * beyond 2^30 frame rows; the overlap. */
int  bsrnn_separate_long_ragged(bsrnn_ctx* ctx, const float* wave_dev, int64_t wave_stride, const int64_t* lens_host,
                                float* wave_out_dev, int32_t R, int32_t seg_frames, void* stream);
/* Frame rows the context's current workspace holds (measurement / test support); 0 before first use, on a host-only context and for
 * a null context.  The workspace is grow-only: this is the largest R * T (or R * seg_frames) any call has needed, rounded up by growth. */
int64_t bsrnn_workspace_rows(const bsrnn_ctx* ctx);

/* ---- validation metrics (m_dataset.py:182-226 `infer` + `train_infer`, infer.py:44-47) ------
 * bsrnn_evaluate: mix_dev [R, n] (the mixture, sample[0]) and speech_dev [R, n] (the clean target,
 * sample[1]) -> separates the mixture (bsrnn_separate) and returns, in metrics_host[BSRNN_N_METRICS]:
 *   LOSS          L1(x_time, s_time) + L1(Re X, Re S) + L1(Im X, Im S), each a mean over its elements
 *                 (train.py:54 L1Loss; no discriminator term), S = STFT of the clean signal;
 *   SDR           mean over rows of 10 log10((sum s^2 + 1e-9) / (sum (x - s)^2 + 1e-9)), s cut to len(x);
 *   INPUT_SDR     the reference's `sdr2` exactly as written: its sample tensors are [1, R, n], so the sums
 *                 run over the R rows and the mean over the n sample positions (m_dataset.py:219-222);
 *   SISDR         scale-invariant SDR of torchmetrics (zero_mean = False, eps = float32 epsilon), mean over rows;
 *   L1_TIME / L1_RE / L1_IM   the three loss terms;
 *   SEPARATION_DB 10 ln(sum mix^2 / sum (mix - x)^2) over all rows (natural log, as infer.py:47 prints it).
 * est_out_dev (optional) receives the separated signal [R, (T-1)*1024]; it must not overlap mix_dev or speech_dev under
 * either policy (BSRNN_EARG: the metrics, and a re-run, read them after the estimate is written).  Synchronous: returns when the
 * numbers are on the host; the call waits once, for the sums.  Reductions accumulate in double on the device; rows are independent,
 * so any R works (the reference's un-interleave hard-codes 2 rows, m_dataset.py:192).  The call is bsrnn_evaluate_ragged's arithmetic
 * on one clip of R rows - the same metric kernels, the same host tail - with bsrnn_separate as its separation.  The sums and, without
 * est_out_dev, the estimate ([R, (T-1)*1024] floats: about 32 MB at 64 rows x 128 000 samples) live in grow-only blocks of the context
 * that the three evaluate calls share: a second call that fits allocates nothing (bsrnn_debug_counter(0)), and the blocks are retained
 * until bsrnn_destroy.  Pass est_out_dev to keep the estimate out of the context. */
#define BSRNN_M_LOSS          0
#define BSRNN_M_SDR           1
#define BSRNN_M_INPUT_SDR     2
#define BSRNN_M_SISDR         3
#define BSRNN_M_L1_TIME       4
#define BSRNN_M_L1_RE         5
#define BSRNN_M_L1_IM         6
#define BSRNN_M_SEPARATION_DB 7
#define BSRNN_N_METRICS       8
int  bsrnn_evaluate(bsrnn_ctx* ctx, const float* mix_dev, const float* speech_dev, int32_t R, int64_t n,
                    float* est_out_dev, double* metrics_host, void* stream);
/* bsrnn_evaluate_ragged = bsrnn_evaluate for n_clips clips of DIFFERENT lengths in one call (a validation set).  The unit of the metrics is
 * a CLIP - one sample of the reference: all rows of one file, all of one length; its validation loop averages per-clip numbers
 * (train.py:132-150) - so the call returns one set of the eight metrics per clip, metrics_host [n_clips][BSRNN_N_METRICS], each what
 * bsrnn_evaluate gives for that clip alone (to rounding: the kernels of the SEPARATION are chosen for the whole batch, so the estimate
 * may differ within the waveform contract; the metric kernels and the host arithmetic behind them are the same).  Nothing is summed across clips:
 * INPUT_SDR sums over the rows of its own clip at each of the clip's sample positions.
 *   - Clip c owns clip_rows_host[c] >= 1 consecutive rows (NULL: one row per clip) of clip_lens_host[c] samples each, 1024 < length <=
 *     wave_stride; R = the sum of the row counts.  mix_dev and speech_dev hold R rows, wave_stride floats apart; what lies behind a row's
 *     samples is never read, in either buffer.
 *   - With n = the clip's length, T = 1 + n / 1024 and n_est = (T - 1) * 1024: the L1 means divide by rows * n_est and rows * 1025 * T,
 *     INPUT_SDR averages over the clip's n positions, SDR and SISDR are means over the clip's rows, SEPARATION_DB runs over the clip's rows.
 *   - est_out_dev (optional) is [R, (Tmax-1)*1024] as bsrnn_separate_ragged writes it (Tmax = the largest T): every row's estimate, then
 *     zeros to the end of the row.  It must not overlap the R * wave_stride floats of mix_dev or speech_dev under either policy (BSRNN_EARG).
 *   - Synchronous; the call waits once, for the partial sums (under BSRNN_RANGE_EXACT bsrnn_separate_ragged inside it waits for the guard as
 *     well).  Range policy as bsrnn_evaluate: the guard is always handled before the numbers return; a re-run repeats the whole flow in
 *     exact fp32 from the same inputs and lengths.
 *   - The two host arrays are the caller's again at return.  The clip table, the partial sums and (without est_out_dev) the estimate live in
 *     grow-only blocks of the context: a second call that fits allocates nothing (bsrnn_debug_counter(0)).  Cost and memory as
 *     bsrnn_separate_ragged: padding is paid for in the model, so batch clips of similar length (the Python layer's evaluate_many does).
 * BSRNN_EARG, before any device work (also on a host-only context, in front of its BSRNN_ESTATE): a null ctx, mix_dev, speech_dev,
 * clip_lens_host or metrics_host; n_clips < 1; a row count < 1; a length <= 1024 or > wave_stride (the text names the clip and the value);
 * R * Tmax beyond bsrnn_separate_ragged's limit. */
int  bsrnn_evaluate_ragged(bsrnn_ctx* ctx, const float* mix_dev, const float* speech_dev, int64_t wave_stride,
                           const int64_t* clip_lens_host, const int32_t* clip_rows_host, int32_t n_clips,
                           float* est_out_dev, double* metrics_host, void* stream);
/* bsrnn_evaluate_long_ragged = bsrnn_evaluate_ragged in segments: clips of DIFFERENT lengths, each of any length, from a workspace of
 * R * min(seg_frames, Tmax) frame rows.  Arguments and result as bsrnn_evaluate_ragged: metrics_host [n_clips][BSRNN_N_METRICS], each clip
 * as bsrnn_evaluate gives it for that clip alone, to rounding.  The separation is bsrnn_separate_long_ragged's - the same cut of the Tmax
 * frames, the alive prefix of the rows (per-clip lengths expanded to rows), carried state and overlap-add tail; bsrnn_debug_counter(4)
 * counts its frame rows, so order the clips LONGEST FIRST.
 *   - seg_frames >= Tmax: the call IS bsrnn_evaluate_ragged (it delegates: numbers and estimate bit-identical).
 *   - Per segment [ta, te): STFT of the mixture on the prefix -> the model -> iSTFT of the segment's hops -> the range guard, handled per
 *     segment under EITHER policy (a segment that left the fp16 range is run again in exact fp32 from its untouched state) -> the clean
 *     signal through the segment's analysis -> the segment's time and spectral sums ADDED into accumulators of a fixed size per row, one
 *     slot per workgroup, in stream order without atomics: run and re-run give the same bits.  INPUT_SDR is formed once over the whole
 *     inputs.  One download at the end; synchronous.
 *   - SISDR is formed from the row's totals instead of a second pass over an estimate that no longer exists: alpha in fp32 as
 *     bsrnn_evaluate forms it, then a^2 sum s^2 over max(0, a^2 sum s^2 - 2 a sum x s + sum x^2) in double (within 4e-7 dB of the two-pass
 *     figure up to 40 dB, 2e-4 dB at 80 dB).
 *   - Memory beyond the two inputs: the workspace of one segment, bsrnn_separate_long_ragged's carry sets, the accumulators, and - without
 *     est_out_dev - an estimate buffer of ONE segment, R * seg_frames * 1024 floats.  Nothing grows with Tmax.  With est_out_dev the
 *     estimate is [R, (Tmax-1)*1024] as bsrnn_separate_long_ragged writes it.  A second call that fits allocates nothing
 *     (bsrnn_debug_counter(0)).
 * BSRNN_EARG, before any device work (also on a host-only context, in front of its BSRNN_ESTATE): everything bsrnn_evaluate_ragged refuses,
 * in its words (the text names the clip); seg_frames < 1; R * min(seg_frames, Tmax) beyond bsrnn_separate_long_ragged's limit;
 * est_out_dev overlapping the R * wave_stride floats of mix_dev or speech_dev, under either policy. */
int  bsrnn_evaluate_long_ragged(bsrnn_ctx* ctx, const float* mix_dev, const float* speech_dev, int64_t wave_stride,
                                const int64_t* clip_lens_host, const int32_t* clip_rows_host, int32_t n_clips,
                                int32_t seg_frames, float* est_out_dev, double* metrics_host, void* stream);

/* ---- ragged training: the clips of one optimizer step in one backward pass -----------------
 * The reference accumulates gradients clip by clip (train.py:97-115).  The same step as ONE rectangle R x Tmax: the model is causal along
 * time, its band-axis blocks see one frame at a time and rows are independent, so a zero-padded rectangle gives every real frame its own
 * result; y = x * mask with x = 0 in the padded frames, so those frames carry neither value nor gradient.  Only the two DSP ends and the
 * loss know the lengths - the five calls below, at the [R, 2050, Tmax] boundary autograd works on (re/im interleaved, T innermost).
 * Conventions as bsrnn_separate_ragged / bsrnn_evaluate_ragged: rows wave_stride floats apart, lens_host[r] samples in row r,
 * 1024 < length <= wave_stride, T_r = 1 + length / 1024, Tmax = the largest T_r, n_est_r = (T_r - 1) * 1024.  The host arrays are the
 * caller's again at return (the lengths travel through the pinned mirrors of bsrnn_separate_ragged's block, in stream order); no call
 * waits for the device and every result stays in device memory, so the calls of one step queue up on ONE stream.  A second step that fits
 * allocates nothing (bsrnn_debug_counter(0)).  No committed weights are needed.
 * BSRNN_EARG, before any device work (also on a host-only context, in front of its BSRNN_ESTATE): a null ctx, buffer or length array;
 * R or n_clips < 1; a row count < 1; a length <= 1024 or > wave_stride (the text names the row or the clip and the value); R * Tmax beyond
 * bsrnn_separate_ragged's limit.
 *
 * bsrnn_stft_ragged: wave_dev -> x_dev [R, 2050, Tmax].  Row r, frames t < T_r: bit-identical to bsrnn_stft of that clip alone (reflect
 *     padding at the clip's own end); frames t >= T_r are written as zeros.
 * bsrnn_istft_ragged: y_dev [R, 2050, Tmax] -> wave_out_dev [R, (Tmax-1)*1024].  Row r gets the n_est_r samples bsrnn_istft gives for
 *     y[r, :, :T_r] (bit-identical), then zeros; what y holds in frames t >= T_r is not used.
 * bsrnn_istft_ragged_backward: the transpose of bsrnn_istft_ragged, row by row.  dwave_dev [R, (Tmax-1)*1024] -> dy_dev [R, 2050, Tmax]:
 *     dy[r, :, t < T_r] is what bsrnn_istft_backward gives for dwave[r, :n_est_r] with T_r frames (the same three passes: bit-identical),
 *     dy[r, :, t >= T_r] = 0, the imaginary parts of bins 0 and 1024 are 0; dwave[r, i >= n_est_r] is never read. */
int  bsrnn_stft_ragged(bsrnn_ctx* ctx, const float* wave_dev, int64_t wave_stride, const int64_t* lens_host, float* x_dev, int32_t R,
                       void* stream);
int  bsrnn_istft_ragged(bsrnn_ctx* ctx, const float* y_dev, const int64_t* lens_host, float* wave_out_dev, int32_t R, void* stream);
int  bsrnn_istft_ragged_backward(bsrnn_ctx* ctx, const float* dwave_dev, const int64_t* lens_host, float* dy_dev, int32_t R, void* stream);
/* bsrnn_train_loss_ragged: the L1 tri-loss and the SDR of `train_infer` (m_dataset.py:202-217) PER CLIP.  Clips as bsrnn_evaluate_ragged's:
 *     clip c owns clip_rows_host[c] >= 1 consecutive rows of clip_lens_host[c] samples (NULL: one row per clip).  y_dev (the model's
 *     output) and s_dev (the clean signal's spectrum) are [R, 2050, Tmax], xtime_dev is [R, (Tmax-1)*1024], speech_dev rows are wave_stride
 *     floats apart.  values_dev, double [n_clips][BSRNN_N_TRAIN_VALUES], receives LOSS, L1_TIME, L1_RE, L1_IM and SDR exactly as
 *     bsrnn_evaluate_ragged defines them for that clip alone (the means divide by rows * n_est and rows * 1025 * T; SDR is the mean over the
 *     clip's rows); row_sums_dev, double [R][2], receives sum s^2 and sum (x - s)^2 of each row for the backward call.  What the tensors
 *     hold behind a row's frames or samples never reaches a result.  Differences in fp32, sums in double in a fixed order: a second run is
 *     bit-identical.
 * bsrnn_train_loss_ragged_backward: the same tensors and tables, row_sums_dev as the forward call left it, and gclip_dev, float
 *     [n_clips][2]: the upstream gradient of each clip's LOSS and of its SDR.  Writes ALL of dy_dev [R, 2050, Tmax] and dxtime_dev
 *     [R, (Tmax-1)*1024]:
 *       dy[r, c, t]  = gL sgn(y - s) / (rows * 1025 * T)                                      for t < T_r, else 0   (sgn(0) = 0)
 *       dxtime[r, i] = gL sgn(x - s) / (rows * n_est) - gS (10 / ln 10) 2 (x - s) / (rows * (sum (x - s)^2_r + 1e-9))   for i < n_est_r, else 0 */
#define BSRNN_TV_LOSS          0
#define BSRNN_TV_L1_TIME       1
#define BSRNN_TV_L1_RE         2
#define BSRNN_TV_L1_IM         3
#define BSRNN_TV_SDR           4
#define BSRNN_N_TRAIN_VALUES   5
int  bsrnn_train_loss_ragged(bsrnn_ctx* ctx, const float* y_dev, const float* s_dev, const float* xtime_dev, const float* speech_dev,
                             int64_t wave_stride, const int64_t* clip_lens_host, const int32_t* clip_rows_host, int32_t n_clips,
                             double* values_dev, double* row_sums_dev, void* stream);
int  bsrnn_train_loss_ragged_backward(bsrnn_ctx* ctx, const float* y_dev, const float* s_dev, const float* xtime_dev,
                                      const float* speech_dev, int64_t wave_stride, const int64_t* clip_lens_host,
                                      const int32_t* clip_rows_host, int32_t n_clips, const double* row_sums_dev, const float* gclip_dev,
                                      float* dy_dev, float* dxtime_dev, void* stream);

/* ---- streaming (infer-streaming.py:84-147; speech-ladspa-onnx.cpp:171-267) -------------
 * A bsrnn_stream owns, on the device, the sliding 2048-sample analysis buffer, the LSTM
 * state [4,2,C*K,64] and the previous synthesis frame for C rows.
 * bsrnn_stream_create does ALL first-use work (allocations, loading every kernel, and - with BSRNN_STREAM_GRAPH=1 - capturing
 * and instantiating the step's hipGraphs: two throw-away steps on zero input, carry zeroed again afterwards), so that the first
 * bsrnn_stream_step* call costs what every later one costs.
 * bsrnn_stream_step: chunk_dev [C, 1024] -> out_dev [C, 1024] (delayed by one chunk; out_dev may overlap chunk_dev, wholly or
 *     partly: under BSRNN_RANGE_EXACT such a chunk is copied aside first, so that a re-run still sees it):
 *     rfft(buf*hann) -> forward_recurrent -> irfft -> 2-slot overlap-add / sum(window).
 * bsrnn_stream_step_host: same with host buffers, synchronous (used by the LADSPA plugin);
 *     `mix` applies the plugin's wet/dry control on the spectrum (speech-ladspa-onnx.cpp:
 *     215-226): mix >= 0: mix*y + (1-mix)*x ; mix < 0: x + mix*y.  Use mix = 1 for
 *     infer-streaming.py semantics. */
int  bsrnn_stream_create(bsrnn_ctx* ctx, int32_t C, bsrnn_stream** out);
void bsrnn_stream_destroy(bsrnn_stream* s);
int  bsrnn_stream_reset(bsrnn_stream* s, void* stream);
int  bsrnn_stream_step(bsrnn_stream* s, const float* chunk_dev, float* out_dev, float mix, void* stream);
int  bsrnn_stream_step_host(bsrnn_stream* s, const float* chunk_host, float* out_host, float mix);
int  bsrnn_stream_get_state(bsrnn_stream* s, float* state_host /* [4,2,C*K,64] */);
/* L = n_hops consecutive bsrnn_stream_step calls in one: chunk_dev [C, n_hops*1024] -> out_dev [C, n_hops*1024]
 * (delayed by one hop, like the step).  Carry (analysis buffer, previous synthesis frame, LSTM state) continues from
 * and for bsrnn_stream_step / _step_host / _process in any mixture.  The model runs once on C * n_hops frame rows, planned
 * like bsrnn_forward_chunk (so a block of several hops agrees with the same hops stepped one by one to rounding, not bit for
 * bit; n_hops = 1 IS the step).  Range policy as for the step; the re-run reads chunk_dev again, so under BSRNN_RANGE_EXACT
 * out_dev must not overlap chunk_dev (BSRNN_EARG); under BSRNN_RANGE_DEFERRED in-place is allowed. */
int  bsrnn_stream_process(bsrnn_stream* s, const float* chunk_dev, float* out_dev, int32_t n_hops, float mix, void* stream);
/* Do now everything a later bsrnn_stream_process of up to max_hops hops would otherwise do at first use (workspace and
 * task tables of C*max_hops frame rows, kernel loading, overlap tables): such calls then allocate, capture and
 * instantiate nothing (bsrnn_debug_counter 0..2 unchanged).  Synchronous; the carry is left as it is. */
int  bsrnn_stream_reserve(bsrnn_stream* s, int32_t max_hops);

/* ---- streaming session slots: hold, reset and move single rows of a bsrnn_stream --------
 * A step is launch-bound (its cost hardly depends on C), so many live sessions are served as a few rows each of ONE wide stream.
 * These calls let the rows of a stream live apart: they join, pause, leave and move one by one.  They take streams of at most
 * BSRNN_STREAM_ROWS_MAX rows (BSRNN_EARG above that; the other stream calls keep their own limits): the set of rows a call means
 * travels by value in the kernel arguments, so no call allocates, stages a copy or keeps anything alive after it returns.
 * bsrnn_stream_process_rows: bsrnn_stream_process for the rows with active_host[r] != 0 (active_host [C] in ordinary host memory, the
 *     caller's again at return under either range policy; NULL = every row).  A held row (active_host[r] == 0) keeps its analysis
 *     buffer, previous synthesis frame and LSTM state bit for bit, its out_dev row is zeros and its chunk_dev row is never read (it may
 *     hold NaN; the row enters the model as a zero spectrum, so stale memory cannot trip the range guard).  An active row gets exactly
 *     the bits the same call with every row active would give it.  mix_rows_dev [C], if not NULL, is a device array of the caller's
 *     with one wet/dry value per row (the formula of bsrnn_stream_step_host; a row at 1 gets the bits of mix = 1) and replaces `mix`; it
 *     must overlap neither chunk_dev nor out_dev.  Every row active and mix_rows_dev == NULL IS bsrnn_stream_process; no row active
 *     zeroes out_dev and does nothing else.  n_hops = 1 takes the step's kernels (and its captured graph, if that is on), more hops the
 *     block path.  Range policy as for bsrnn_stream_process, held rows staying held through a re-run; under BSRNN_RANGE_EXACT out_dev
 *     must not overlap chunk_dev for any n_hops (BSRNN_EARG).  Costs no launch more than the plain call.
 * bsrnn_stream_reset_rows: zeroes the carry of the n_rows rows listed in rows_host (each in [0, C); BSRNN_EARG names a bad one), in
 *     stream order and one launch: the next hops of such a row are those of the same row of a freshly created stream of the same C.
 * bsrnn_stream_row_floats: floats of one row's carry, 2*2048 + 8*K*64 (-1 for a null stream).
 * bsrnn_stream_get_row / _set_row: synchronous; copy one row's carry to / from blob_host [buf 2048 | prev 2048 | state 4,2,K,64].  A
 *     blob set into any row of a stream of the same C and band table continues bit for bit as it would have in place.  get_row reports
 *     a range violation left by calls under BSRNN_RANGE_DEFERRED, like bsrnn_stream_get_state.
 * bsrnn_stream_process_hops: one call in which every row advances by its OWN number of hops - what a server needs whose sessions do
 *     not deliver audio in lock step.  Buffers as for bsrnn_stream_process_rows: chunk_dev and out_dev are [C, n_hops*1024]; hops_host
 *     [C] (ordinary host memory, each in [0, n_hops], the caller's again at return under either range policy) says how far each row
 *     goes.  Row r with h = hops_host[r]: its first h*1024 samples of chunk_dev are read and nothing behind them (it may hold NaN); its
 *     first h*1024 samples of out_dev are what h consecutive bsrnn_stream_step calls would give that row, the rest of its out_dev row is
 *     zeros; its carry (analysis buffer, previous synthesis frame, LSTM state) is the carry after exactly h hops.  h = 0 holds the row
 *     as bsrnn_stream_process_rows does: carry bit for bit as it was.  The counts travel by value in the kernel arguments (8 bits per
 *     row: at most BSRNN_STREAM_HOPS_MAX hops per call), so the call allocates nothing, stages no copy and keeps nothing alive.
 *     When every count is 0 or n_hops the call IS bsrnn_stream_process_rows with active = hops != 0 (bit-identical by construction,
 *     one-hop path included; no row with a hop: out_dev zeroed, nothing else).  Mixed counts always take the block path: the model runs
 *     on all C * n_hops frame rows (a row's frames past its count enter it as zero spectra), planned exactly as the plain call, and its
 *     time-axis launches hand back each row's LSTM state after that row's last frame.  The frames of a row below its count are
 *     those of a call in which the row has all n_hops hops of the same leading audio: the time axis is causal, all else is per frame.
 *     mix_rows_dev, mix, range policy (a re-run keeps the counts), the overlap rules and the concurrency contract: as
 *     bsrnn_stream_process_rows.  After bsrnn_stream_reserve(max_hops) - or after the first hops call of a shape - hops calls of up to
 *     max_hops hops allocate, capture and instantiate nothing, whatever the counts.
 *     BSRNN_EARG, the text naming the problem: a null s, chunk_dev, out_dev or hops_host; n_hops outside [1, BSRNN_STREAM_HOPS_MAX];
 *     a count outside [0, n_hops] (the row is named); more than BSRNN_STREAM_ROWS_MAX rows; the overlaps above. */
#define BSRNN_STREAM_ROWS_MAX 2048
#define BSRNN_STREAM_HOPS_MAX 255
int     bsrnn_stream_process_rows(bsrnn_stream* s, const float* chunk_dev, float* out_dev, int32_t n_hops,
                                  const uint8_t* active_host, const float* mix_rows_dev, float mix, void* stream);
int     bsrnn_stream_process_hops(bsrnn_stream* s, const float* chunk_dev, float* out_dev, int32_t n_hops,
                                  const int32_t* hops_host, const float* mix_rows_dev, float mix, void* stream);
int     bsrnn_stream_reset_rows(bsrnn_stream* s, const int32_t* rows_host, int32_t n_rows, void* stream);
int64_t bsrnn_stream_row_floats(const bsrnn_stream* s);
int     bsrnn_stream_get_row(bsrnn_stream* s, int32_t row, float* blob_host);
int     bsrnn_stream_set_row(bsrnn_stream* s, int32_t row, const float* blob_host);

/* ---- sample-rate conversion on the device ------------------------------------------------
 * The model is trained on 44.1 kHz audio; these calls bring audio of another rate to it and back without leaving the device.  They replace
 * the host-side resampling in front of the reference's loops: `torchaudio.functional.resample` at infer-streaming.py:77-78 / the
 * `sample_rate=44100` its StreamReader asks ffmpeg for, and what a caller of infer.py has to do to a 48 kHz file beforehand.
 * DEFINITION: exactly scipy.signal.resample_poly(x, up, down) with its defaults (zero phase, zeros outside the clip), the project's own
 * host behaviour until now (speechseparation_amd/audio.py:resample).  g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g,
 * M = max(up, down), half = 10 * M, taps h = firwin(2 * half + 1, 1 / M, window = ('kaiser', 5.0)) * up designed in double and rounded to
 * fp32 once, n_out = ceil(n_in * up / down), y[j] = sum_i x[i] * h[j * down - i * up + half] over the i inside the clip and the filter;
 * fp32 accumulation.  Parity with ffmpeg's (or torchaudio's) resampler is NOT pinned: their filters differ from scipy's.
 * Limits (BSRNN_EARG, the text names the value; answered before anything touches a device, also on a host-only context in front of its
 * BSRNN_ESTATE): a rate < 1; a reduced max(up, down) > 1024 (44.1 kHz to and from 8 / 11.025 / 12 / 16 / 22.05 / 24 / 32 / 48 / 88.2 / 96 /
 * 176.4 / 192 kHz all fit: 441 or 640 at most); n_in < 1.
 * bsrnn_resample_len: n_out for n_in samples, or -1 for arguments bsrnn_resample would refuse.  Needs no context.
 * bsrnn_resample: in_dev holds R rows in_stride floats apart with n_in samples each (nothing behind them in a row is read) -> out_dev, R rows
 *     out_stride floats apart, n_out samples each (nothing behind them in a row is written): the strides fit the padded buffers of the
 *     ragged calls.  Enqueues and returns.  Equal rates make the call a copy.  out_dev (its (R - 1) * out_stride + n_out floats) must not
 *     overlap the (R - 1) * in_stride + n_in floats that the rows of in_dev span - first sample of the first row to last sample of the last,
 *     the padding between rows included, the padding behind the last row not: it may belong to another allocation - and a stride must hold
 *     its row (BSRNN_EARG).  The polyphase table of a rate pair is built and uploaded when the context first meets the
 *     pair (bsrnn_debug_counter(0)); it needs no committed weights.  Counts as a call on the context (concurrency contract above).
 * A bsrnn_resampler converts a stream block by block.  It holds, on the device and per row, the input samples that later outputs still
 *     need (at most 2 * half / up + down / up + 2 floats); its two sample counters live on the host.
 *   bsrnn_resampler_create does all first-use work (table, carry, kernel loading); _process, _flush and _reset allocate nothing
 *     (bsrnn_debug_counter(0) unchanged).  Lifetime against bsrnn_destroy as a bsrnn_stream's: the context is released with the last object.
 *   bsrnn_resampler_process: in_dev [C rows, in_stride apart, n_in samples], any n_in >= 0 -> writes to out_dev [C rows, out_stride apart]
 *     exactly the outputs that have become determined - those whose last input has arrived - and reports their count per row in
 *     *n_out_host without synchronising (the count is host arithmetic: bsrnn_resampler_ready(r, n_in) gives it beforehand, -1 for a
 *     null object or n_in < 0).  out_dev must not overlap in_dev and out_stride must hold the count (BSRNN_EARG).
 *   bsrnn_resampler_flush: writes the rest, up to ceil(N * up / down) for the N samples taken, the future counting as zeros, and leaves the
 *     object reset.  bsrnn_resampler_reset: forget the stream so far (host only; nothing is enqueued).
 *   The concatenated outputs of any sequence of _process calls and one _flush EQUAL bsrnn_resample of the concatenated input, value for
 *     value: one kernel forms an output sample from the same taps in the same order wherever its inputs lie. */
typedef struct bsrnn_resampler bsrnn_resampler;
int64_t bsrnn_resample_len(int64_t n_in, int32_t rate_in, int32_t rate_out);
int     bsrnn_resample(bsrnn_ctx* ctx, const float* in_dev, int64_t in_stride, float* out_dev, int64_t out_stride,
                       int32_t R, int64_t n_in, int32_t rate_in, int32_t rate_out, void* stream);
int     bsrnn_resampler_create(bsrnn_ctx* ctx, int32_t C, int32_t rate_in, int32_t rate_out, bsrnn_resampler** out);
void    bsrnn_resampler_destroy(bsrnn_resampler* r);
int     bsrnn_resampler_reset(bsrnn_resampler* r, void* stream);
int64_t bsrnn_resampler_ready(const bsrnn_resampler* r, int64_t n_in);
int     bsrnn_resampler_process(bsrnn_resampler* r, const float* in_dev, int64_t in_stride, int64_t n_in,
                                float* out_dev, int64_t out_stride, int64_t* n_out_host, void* stream);
int     bsrnn_resampler_flush(bsrnn_resampler* r, float* out_dev, int64_t out_stride, int64_t* n_out_host, void* stream);

/* ---- a bank of streaming resamplers: a rate pair, a block length and a stream position PER ROW ----
 * A bsrnn_resampler has one rate pair and moves all its rows in lock step.  A bsrnn_resampler_bank holds C rows that each sit on one of up
 * to BSRNN_BANK_PAIRS_MAX declared rate pairs, at their own place in their own stream, and converts all of them in ONE launch-bound call:
 * what a pool of live sessions at 8, 16, 32, 48 and 96 kHz needs in front of and behind one bsrnn_stream_process_hops (one bank into the
 * model's 44.1 kHz, one out of it), instead of two bsrnn_resampler calls per session.
 * DEFINITION: row r of a bank IS a one-row bsrnn_resampler of r's pair.  Counts and samples are equal value for value - the same kernel
 * code forms an output sample from the same taps in the same order - so the concatenated outputs of a row, flush included, equal
 * bsrnn_resample of the row's concatenated input.
 * Limits (BSRNN_EARG, the text names the value; answered before anything touches a device): a null object; a row outside [0, C) or listed
 * twice; a pair outside [0, n_pairs); n_pairs outside [1, BSRNN_BANK_PAIRS_MAX]; a rate pair bsrnn_resample would refuse; a count < 0, or
 * more than 2^30 samples into or out of one row in one call; in_stride below the largest count given; out_stride below the largest count
 * written; out_dev overlapping the span of in_dev.
 *   bsrnn_resampler_bank_create does all first-use work - the tables of all declared pairs (shared with the context's other resampling
 *     calls), the carry (two sets of C x cap floats, cap the largest carry of the declared pairs), the pair table on the device, kernel
 *     loading; every other call allocates nothing (bsrnn_debug_counter(0) unchanged).  All rows start on pair 0 at the beginning of a
 *     stream.  Lifetime against bsrnn_destroy as a bsrnn_resampler's.
 *   bsrnn_resampler_bank_assign: the listed rows move to declared pair `pair` and start a new stream there.  _reset_rows: the listed rows
 *     start a new stream on the pair they have.  Both are host-only (nothing is enqueued: with no input taken a row's carry holds no sample
 *     a call would read).  _pair_of: a row's pair, -1 for a null object or a row outside [0, C).
 *   bsrnn_resampler_bank_ready: the count the next _process would report for `row` if it gave the row n_in samples; -1 for a null object, a
 *     row outside [0, C) or n_in < 0.
 *   bsrnn_resampler_bank_process: row r reads its first n_in_host[r] samples of in_dev [C rows, in_stride apart] and nothing behind them;
 *     a count of 0 HOLDS the row - nothing of it is read or written, its carry stays.  Each row gets exactly the outputs that have
 *     become determined, out_dev[r][0 .. n_out_host[r]), and nothing behind them is written; the counts are host arithmetic, reported
 *     without synchronising.  Enqueues and returns: the per-row descriptors travel by value in the kernel arguments, so n_in_host and
 *     n_out_host are the caller's own again at return.  One launch per 179 rows.
 *   bsrnn_resampler_bank_flush_rows: the listed rows get what they are still owed - up to ceil(N * up / down) for the N samples a row
 *     took, the future counting as zeros - and are left at the beginning of a stream; the other rows are untouched and report 0.
 *   A bank call counts as a call on the context (concurrency contract above). */
#define BSRNN_BANK_PAIRS_MAX 16
typedef struct bsrnn_resampler_bank bsrnn_resampler_bank;
int     bsrnn_resampler_bank_create(bsrnn_ctx* ctx, int32_t C, const int32_t* rates_in_host, const int32_t* rates_out_host,
                                    int32_t n_pairs, bsrnn_resampler_bank** out);
void    bsrnn_resampler_bank_destroy(bsrnn_resampler_bank* b);
int     bsrnn_resampler_bank_assign(bsrnn_resampler_bank* b, const int32_t* rows_host, int32_t n_rows, int32_t pair);
int     bsrnn_resampler_bank_pair_of(const bsrnn_resampler_bank* b, int32_t row);
int64_t bsrnn_resampler_bank_ready(const bsrnn_resampler_bank* b, int32_t row, int64_t n_in);
int     bsrnn_resampler_bank_process(bsrnn_resampler_bank* b, const float* in_dev, int64_t in_stride, const int64_t* n_in_host,
                                     float* out_dev, int64_t out_stride, int64_t* n_out_host, void* stream);
int     bsrnn_resampler_bank_flush_rows(bsrnn_resampler_bank* b, const int32_t* rows_host, int32_t n_rows,
                                        float* out_dev, int64_t out_stride, int64_t* n_out_host, void* stream);
int     bsrnn_resampler_bank_reset_rows(bsrnn_resampler_bank* b, const int32_t* rows_host, int32_t n_rows);

/* ---- a pool of live sessions: one call per tick, a pointer per session ------------------------
 * What a many-session server needs on top of bsrnn_stream_process_hops, as an object of the library: `slots` sessions of rows_per_session
 * rows each on ONE wide bsrnn_stream of C = slots * rows_per_session rows (session in slot k owns rows k * rows_per_session ...), a
 * device-resident FIFO per row for the samples that do not yet fill a hop, and ONE call per tick that takes whatever every session has.
 * bsrnn_pool_feed: session i of the call (i < n_sessions; all arrays [n_sessions], ordinary host memory, the caller's again at return under
 *     either range policy) sits in open slot slots_host[i] and brings n_in[i] >= 0 samples per row at in_dev[i], its rows in_stride[i] floats
 *     apart (a null pointer is fine with n_in = 0).  With p = bsrnn_pool_pending(slot) it has h = (p + n_in[i]) / 1024 hops in hand: it gets
 *     n_out_host[i] = h * 1024 samples per row at out_dev[i], rows out_stride[i] floats apart - exactly what h consecutive bsrnn_stream_step
 *     calls give its rows for the stream FIFO ++ input, delayed by one hop - and nothing behind them is written; the remaining
 *     (p + n_in[i]) % 1024 samples wait in the FIFO.  n_out_host is host arithmetic, filled at return without synchronising.  Only 4-byte
 *     alignment of pointers and strides is assumed.  Sessions not named are held (bsrnn_stream_process_rows).
 *     The call runs in rounds of at most max_hops hops: per round one gather launch (FIFO ++ input into the pool's own [C, L*1024]
 *     rectangle, zeros behind a row's hops, and what stays waiting into the FIFO), ONE bsrnn_stream_process_hops(n_hops = L = the most hops
 *     anyone still has, capped at max_hops; a session's count is what it has left, capped at L; everyone else 0), one scatter launch, all
 *     on the caller's stream.  If nobody has a hop the call is the one gather launch.  n_sessions == 0 does nothing.
 *     mix_host == NULL: every row takes the scalar `mix` (bsrnn_stream_step_host's formula; 1 for plain separation).  Otherwise mix_host[i]
 *     is session i's value and the rows of everybody else are at 1; `mix` is ignored.
 *     Range policy: as bsrnn_stream_process_hops - under BSRNN_RANGE_DEFERRED the call waits for nothing; under BSRNN_RANGE_EXACT it waits in
 *     every round as the hops call does, and a re-run reads the pool's rectangle again: the FIFO is consumed once.
 *     BSRNN_EARG before any device work, the pool untouched, the text naming the session: a null pool or array; a slot that is not open or
 *     named twice; n_in < 0; in_stride below n_in; out_stride below n_out; a null pointer where samples are to be read or written; ANY
 *     output range of the call overlapping ANY input range of the call (a later round reads input behind what an earlier round has
 *     written, so in place is not offered).
 * bsrnn_pool_feed_host: the same with in / out in ordinary host memory, synchronous: per round the sessions' samples are copied into a
 *     pinned block, go up in one copy, the same three launches run, the result comes down in one copy and is handed out.  The same
 *     arithmetic: bit-identical to the device form.  Behaves as under BSRNN_RANGE_EXACT (it waits anyway).
 * bsrnn_pool_create does ALL first-use work: the stream and bsrnn_stream_reserve(max_hops), the two rectangles, the FIFOs, the table
 *     block (one entry per row and a wet / dry value per row, with pinned mirrors used in turn) and the host form's pinned staging with its
 *     device mirrors.  Afterwards no feed allocates, captures or instantiates (bsrnn_debug_counter 0..2 unchanged).  BSRNN_EARG for
 *     C > BSRNN_STREAM_ROWS_MAX or max_hops outside [1, BSRNN_STREAM_HOPS_MAX].  bsrnn_pool_destroy also destroys the stream.
 * bsrnn_pool_open: the lowest free slot; its rows start from silence (reset in the order of the stream the pool was last fed on) and
 *     nothing waits.  bsrnn_pool_close frees a slot; what waited is dropped.  bsrnn_pool_pending: samples per row waiting, < 1024; -1 for
 *     a null pool or a slot that is not open.
 * bsrnn_pool_stream: the wide stream, for bsrnn_stream_get_row / _set_row of a session's rows.  With bsrnn_pool_get_pending /
 *     _set_pending (synchronous; host [rows_per_session, 1024], the first n floats of each row count, n < 1024) a session moves between
 *     pools in the middle of a hop and continues bit for bit.
 * A pool call counts as a call on the context (concurrency contract above). */
typedef struct bsrnn_pool bsrnn_pool;
int     bsrnn_pool_create(bsrnn_ctx* ctx, int32_t slots, int32_t rows_per_session, int32_t max_hops, bsrnn_pool** out);
void    bsrnn_pool_destroy(bsrnn_pool* p);
int     bsrnn_pool_open(bsrnn_pool* p, int32_t* slot_out);
int     bsrnn_pool_close(bsrnn_pool* p, int32_t slot);
int64_t bsrnn_pool_pending(const bsrnn_pool* p, int32_t slot);
bsrnn_stream* bsrnn_pool_stream(bsrnn_pool* p);
int     bsrnn_pool_get_pending(bsrnn_pool* p, int32_t slot, float* host, int32_t* n);
int     bsrnn_pool_set_pending(bsrnn_pool* p, int32_t slot, const float* host, int32_t n);
int     bsrnn_pool_feed(bsrnn_pool* p, int32_t n_sessions, const int32_t* slots_host, const float* const* in_dev, const int64_t* in_stride,
                        const int64_t* n_in, float* const* out_dev, const int64_t* out_stride, int64_t* n_out_host,
                        const float* mix_host, float mix, void* stream);
int     bsrnn_pool_feed_host(bsrnn_pool* p, int32_t n_sessions, const int32_t* slots_host, const float* const* in_host,
                             const int64_t* in_stride, const int64_t* n_in, float* const* out_host, const int64_t* out_stride,
                             int64_t* n_out_host, const float* mix_host, float mix);

/* ---- sessions of a pool at their own sample rates -----------------------------------------------
 * bsrnn_pool_create_rates: a pool whose sessions may give and get audio at one of n_rates declared rates (rates_host [n_rates], n_rates in
 *     [1, BSRNN_BANK_PAIRS_MAX], each a rate bsrnn_resample converts to and from the model's 44100).  max_block: the most samples per row,
 *     at its own rate, such a session brings in one feed.  It does ALL first-use work of such a pool on top of bsrnn_pool_create's: the
 *     tables and carries of an inbound bank (rate -> 44100) and an outbound bank (44100 -> rate) of C rows each, two staging rectangles
 *     conv_in / conv_out [C, cap] (cap: what max_block samples make at 44.1 kHz, and what a drain needs, in whole hops) and a larger table
 *     block.  Afterwards bsrnn_debug_counter(0..2) do not move through feeds and drains.
 * bsrnn_pool_open_rate: bsrnn_pool_open for a session at sample_rate; 44100 gives a plain session (so does bsrnn_pool_open).  Host-only
 *     apart from the stream-row reset bsrnn_pool_open makes: the slot's rows of both banks are assigned their pair and start afresh.
 *     bsrnn_pool_close resets them.  bsrnn_pool_rate_of: the session's rate; -1 for a null pool or a slot that is not open.
 * bsrnn_pool_feed with such a session: n_in[i] counts samples AT ITS RATE (at most max_block), n_out_host[i] is what
 *     bsrnn_pool_ready(pool, slot, n_in[i]) reports beforehand - the output samples at its rate that have become determined, a count that
 *     varies from tick to tick - and out_stride[i] must hold that count.  The tick: ONE inbound bank launch for all such sessions that
 *     bring samples (session pointers -> conv_in, a rate pair, a count and a stream position per row), the rounds as above with conv_in
 *     and conv_out in the place of these sessions' pointers, ONE outbound bank launch (conv_out -> session pointers): 2 + 3 * rounds
 *     launches.  The stream's one-hop delay is taken out of such a session's audio: the first hop after open or drain is not handed on.
 *     bsrnn_pool_pending stays "samples at the MODEL's rate waiting, < 1024".  A feed that names no such session makes exactly the calls
 *     it made before.  Under BSRNN_RANGE_EXACT a re-run reads the pool's rectangle again: FIFO, bank carries, positions and the dropped
 *     hop advance once.  Bit for bit what a pool without rates gives with a single-pair bsrnn_resampler per session and direction
 *     around it (bsrnn_resampler_process of every tick's chunk, the first hop dropped, bsrnn_resampler_process of the result).
 *     Further refusals (BSRNN_EARG before any device work, the pool untouched, the session named): n_in above max_block; the overlap
 *     check uses the real n_out.  bsrnn_pool_feed_host refuses a session with a rate.
 * bsrnn_pool_ready: n_out the next feed of n_in samples would report for the slot (any session); -1 for a null pool, a slot that is
 *     not open, n_in < 0 or above max_block.  bsrnn_pool_drain_len: what bsrnn_pool_drain would give now; -1 likewise.
 * bsrnn_pool_drain: the session's audio ends; out_dev (rows out_stride >= the count apart) gets the tail it is still owed and
 *     *n_out_host the count.  In order, every other session held: the inbound rows are flushed, what waits is padded with zeros to a whole
 *     hop, one more hop of zeros follows for the stream's delay, those hops run (in rounds), the outbound rows take them and are flushed.
 *     The slot stays open: its stream rows are reset in the stream's order, both bank rows are reset, the next hop is dropped again and
 *     nothing is pending.  A session that fed n samples at rate r since open or drain has received, feeds and tail together,
 *     bsrnn_resample_len(m, 44100, r) samples with m = bsrnn_resample_len(n, r, 44100) rounded up to whole hops.  A plain session drains
 *     too, in a pool of either kind: the padded hops and one more, as the stream gives them.  mix: the scalar of bsrnn_pool_feed.
 *     BSRNN_EARG: a null pool or argument, a slot that is not open, out_stride below the count. */
int     bsrnn_pool_create_rates(bsrnn_ctx* ctx, int32_t slots, int32_t rows_per_session, int32_t max_hops, const int32_t* rates_host,
                                int32_t n_rates, int64_t max_block, bsrnn_pool** out);
int     bsrnn_pool_open_rate(bsrnn_pool* p, int32_t sample_rate, int32_t* slot_out);
int32_t bsrnn_pool_rate_of(const bsrnn_pool* p, int32_t slot);
int64_t bsrnn_pool_ready(const bsrnn_pool* p, int32_t slot, int64_t n_in);
int64_t bsrnn_pool_drain_len(const bsrnn_pool* p, int32_t slot);
int     bsrnn_pool_drain(bsrnn_pool* p, int32_t slot, float* out_dev, int64_t out_stride, int64_t* n_out_host, float mix, void* stream);

/* ---- long FIR convolution of ragged rows (room impulse responses) ------------------------
 * The reference applies a room impulse response to a training clip with torch.nn.functional.conv1d(x, h, padding='same') and
 * the whole response as the kernel (m_dataset.py:92-114).  These calls compute the same function - for a row x of n samples
 * and a filter h of k taps, left = (k - 1) / 2:
 *     y[m] = sum_{j < k} x[m + j - left] * h[j],   x = 0 outside [0, n),   m in [0, n)
 * (a cross-correlation; the extra sample of padding is on the right for even k) - as a uniformly partitioned overlap-save
 * convolution on the library's 2048-point transform, for rows of different lengths and different filters in one call.
 * Against the float64 definition the result is within a few 1e-7 of the output's peak for 1 ... 262144 taps.
 *
 * A bank (the create call) holds n_filters filters, 1 <= n_taps <= 262144 each, given as host arrays; the partition spectra
 * are built on the device once, here (synchronous).  On a host-only context the bank holds the tap counts only: the count
 * and taps queries answer, the convolve call checks its arguments and then returns BSRNN_ESTATE.  A bank keeps its context
 * alive like a stream does.  The taps query returns -1 for a filter outside [0, count).
 *
 * The convolve call writes out_dev[r * out_stride + m], m < lens_host[r], = row r of in_dev (rows in_stride floats apart)
 * under filter filter_host[r]; a filter of -1 copies the row unchanged, bit for bit.  Samples of out_dev past lens_host[r]
 * are not touched, in_dev is not written.  A row's bits depend on the row, its length and its filter alone - not on the
 * other rows of the call, on R or on the strides.  lens_host and filter_host are free when the call returns; the call is
 * asynchronous on `stream`.  Refused with BSRNN_EARG and a sentence that names the argument: a null pointer, R < 1, a
 * length < 1 (or > 2^40), a stride shorter than a length, a filter outside [-1, count), out_dev overlapping the floats
 * the rows of in_dev span, and in_dev / out_dev on another device than the bank's context.  Workspace: two buffers of
 * spectra (2050 floats per 1024 samples of every row, and per partition of overhang), grow-only, held by the context; a
 * call whose rows need more than 65536 spectra per buffer (0.5 GB) runs as consecutive row groups, with the same bits. */
typedef struct bsrnn_fir_bank bsrnn_fir_bank;
int     bsrnn_fir_bank_create(bsrnn_ctx* ctx, int32_t n_filters, const float* const* taps_host, const int32_t* n_taps_host, bsrnn_fir_bank** out);
void    bsrnn_fir_bank_destroy(bsrnn_fir_bank* bank);
int32_t bsrnn_fir_bank_count(const bsrnn_fir_bank* bank);
int32_t bsrnn_fir_bank_taps(const bsrnn_fir_bank* bank, int32_t filter);
int     bsrnn_convolve_ragged(bsrnn_fir_bank* bank, const float* in_dev, int64_t in_stride, const int64_t* lens_host,
                              const int32_t* filter_host, float* out_dev, int64_t out_stride, int32_t R, void* stream);

/* ---- the streaming (hop-by-hop) form of the FIR convolution ---------------------------------
 * A bsrnn_fir_stream has C rows on one bsrnn_fir_bank.  Each row sits on one filter of the bank, or on -1 (bypass), and at its own place
 * in its own stream: a live recording that arrives in windows is reverberated as it comes, instead of being buffered to its end.
 * DEFINITION, for a row on a filter of k taps that has taken N samples so far, with B = 1024: the row has been handed exactly
 *     E(N) = max(0, floor(N / B) * B - shift)
 * output samples; a flush hands out the remaining N - E(N) and leaves the row at the beginning of a stream.
 *   BSRNN_FIR_SAME, shift = k / 2: the concatenated output of a row, flush included, equals bsrnn_convolve_ragged of the concatenated
 *     input under the same filter BIT FOR BIT, for every way of cutting the input into calls (counts of 0 included) - the same
 *     transforms, and the partitions summed in the same order with the same fused multiply-adds.
 *   BSRNN_FIR_CAUSAL, shift = 0: y[m] = sum_{j < k} x[m - (k - 1) + j] * h[j], m < N - no output sample depends on a later input
 *     sample, and the latency is under one hop instead of k / 2 samples.  A host that wants y = x * r for a response r gives the bank r
 *     reversed.  The flush ends the row at N samples as the one-shot ends a row; a reverb tail past the end is what feeding zeros in
 *     front of the flush gives.  The alignment belongs to the stream (chosen at creation), not to a row.
 *   A bypass row (filter -1) hands out the samples it is given, bit for bit, in the same call (ready = n_in); its flush gives 0.
 * The hot case is a tick - many rows, one hop each: ONE launch per call, one workgroup per row.  Bulk feeding (few rows, many hops per
 * call) is correct but serial per row; bsrnn_convolve_ragged remains the fast path for whole rows.
 * Limits (BSRNN_EARG, the text names the value; answered before any device work, the object untouched): a null object, array or pointer;
 * C < 1; max_taps outside [1, 262144]; align outside {0, 1}; a row outside [0, C) or listed twice; a filter outside [-1, count); a
 * filter with more taps than max_taps; a count < 0 or > 2^30; a stride below the largest count read or written; out_dev overlapping the
 * span of in_dev; pointers on another device than the context's.  On a host-only context the argument checks and the count queries
 * answer, and then BSRNN_ESTATE, as for the bank.
 *   bsrnn_fir_stream_create does all first-use work - the ring of the last conv_partitions(max_taps) input spectra per row
 *     ([C][ceil(max_taps / 1024)][2050] floats), the previous 1024 inputs and a FIFO of < 1024 samples per row, the table block, the
 *     kernel's first launch; afterwards bsrnn_debug_counter(0) does not move through process and flush.  All rows start on bypass.  The
 *     stream keeps its bank alive (a bank destroyed before its last stream goes with that stream), and through the bank the context.
 *   bsrnn_fir_stream_assign: the listed rows move to `filter` and start a new stream there.  _reset_rows: the listed rows start a new
 *     stream on the filter they have.  Both are host-only (a row at the beginning of a stream reads nothing an earlier one left).
 *     _filter_of: a row's filter; -2 for a null object or a row outside [0, C).
 *   bsrnn_fir_stream_ready: the count the next _process would report for `row` if it gave the row n_in samples; -1 for a null object, a
 *     row outside [0, C), n_in < 0 or n_in > 2^30.
 *   bsrnn_fir_stream_process: row r reads its first n_in_host[r] samples of in_dev [C rows, in_stride apart] and nothing behind them; a
 *     count of 0 HOLDS the row.  Every row is written exactly n_out_host[r] samples, out_dev[r][0 .. n_out_host[r]), and nothing behind
 *     them; the counts are host arithmetic, reported without synchronising.  Asynchronous on `stream`; n_in_host and n_out_host are the
 *     caller's own again at return.
 *   bsrnn_fir_stream_flush_rows: the listed rows get what they are still owed and are left at the beginning of a stream; the other rows
 *     are untouched and report 0.
 *   A stream call counts as a call on the context (concurrency contract above). */
typedef struct bsrnn_fir_stream bsrnn_fir_stream;
#define BSRNN_FIR_SAME 0
#define BSRNN_FIR_CAUSAL 1
int     bsrnn_fir_stream_create(bsrnn_fir_bank* bank, int32_t C, int32_t max_taps, int32_t align, bsrnn_fir_stream** out);
void    bsrnn_fir_stream_destroy(bsrnn_fir_stream* s);
int     bsrnn_fir_stream_assign(bsrnn_fir_stream* s, const int32_t* rows_host, int32_t n_rows, int32_t filter);
int32_t bsrnn_fir_stream_filter_of(const bsrnn_fir_stream* s, int32_t row);
int64_t bsrnn_fir_stream_ready(const bsrnn_fir_stream* s, int32_t row, int64_t n_in);
int     bsrnn_fir_stream_process(bsrnn_fir_stream* s, const float* in_dev, int64_t in_stride, const int64_t* n_in_host,
                                 float* out_dev, int64_t out_stride, int64_t* n_out_host, void* stream);
int     bsrnn_fir_stream_flush_rows(bsrnn_fir_stream* s, const int32_t* rows_host, int32_t n_rows,
                                    float* out_dev, int64_t out_stride, int64_t* n_out_host, void* stream);
int     bsrnn_fir_stream_reset_rows(bsrnn_fir_stream* s, const int32_t* rows_host, int32_t n_rows);

/* ---- dialog / background section mining ---------------------------------------------------
 * The reference's gendataset-separate.py runs the separator over a long recording, forms two figures for every hop of 1024
 * samples (:100-105) and cuts the recording into dialog and background sections with a run-length state machine (:111-149);
 * those files are what MixDataSet trains on.  bsrnn_hop_activity forms the figures on the device for a ragged batch,
 * bsrnn_sections_scan is the state machine, a plain host function.
 *
 * bsrnn_hop_activity: row r has hops_host[r] hops (NULL: every row has Hmax).  Hop h of row r covers, for j = 0 ... 1023,
 *     e[j] = est_dev[r * est_stride + h * 1024 + j],   w[j] = mix_dev[r * mix_stride + h * 1024 + j]
 * and with, all rounded to fp32 exactly where the reference's tensors are, b = w - e, q = (e * e) / (b * b) (three roundings,
 * IEEE division) and s = w * w, the sums of the 1024 q and of the 1024 s are formed in double and
 *     act_dev[(r * Hmax + h) * 2 + BSRNN_ACT_RATIO] = sum q / 1024,     ... + BSRNN_ACT_LEVEL] = sum s / 1024
 * are stored: raw means, not dB - thresholds stay on the host.  IEEE special values pass through: one sample with b == 0 and
 * e != 0 makes the hop's ratio +inf, 0 / 0 makes it NaN (digital silence), an all-zero estimate gives exactly 0.  All of
 * act_dev [R][Hmax][2] is written, the slots at and behind a row's hop count as (0, 0).  Nothing behind hops_host[r] * 1024
 * samples of a row is read, in either buffer.  Rounding: a sum differs from the exactly ordered float64 sum of the same fp32
 * terms by at most 1023 * 2^-53 relative; a row's values depend on the row alone, and rows whose bases and strides allow
 * 16-byte loads give the same bits as rows that do not.
 * The call is asynchronous on `stream`, needs no committed weights, and allocates nothing once a call of its size has been
 * made (bsrnn_debug_counter(0)); hops_host is the caller's again at return.
 * The estimate and the mixture are compared sample for sample as given.  A comparison against later or earlier input is the
 * caller's pointer arithmetic, not a parameter: the reference's loop subtracts its streaming separator's output - which is
 * late (the overlap-add of gendataset-separate.py:63-78 completes a chunk only after later ones have come in) - from the
 * CURRENT input chunk (:99-101), an artefact of that delay.  This library's streams are one hop late (bsrnn_stream_step).
 * With est_dev the L hops a stream returned for the L hops at `input`: est_dev + 1024, mix_dev = input and L - 1 hops
 * compare aligned signals (output hop k + 1 is input hop k); est_dev and mix_dev = input as they are reproduce the
 * reference's pairing of a late estimate with the current chunk.
 * Refused with BSRNN_EARG before any device work - on a host-only context in front of its BSRNN_ESTATE: a null ctx, buffer
 * or act_dev; R < 1 or Hmax < 1; a stride < Hmax * 1024; a hop count < 0 or > Hmax (the text names the row and the value);
 * act_dev overlapping the floats the rows of either input span.
 *
 * The rule (bsrnn_section_rule; bsrnn_section_rule_default fills in the reference's constants: 10, 3, -30, -100, 1e-10,
 * -200, 10), per hop:  db = 10 ln(ratio) and level = floor_db if level_mean < level_floor, else 10 ln(level_mean) - natural
 * logs, as the reference writes them.  A ratio of exactly 0 gives db = -inf: the reference's math.log(0) raises there, the
 * one deliberate deviation.  +inf and NaN pass through; a NaN db fails every comparison, so such a hop can only bridge
 * (through its level) or reset.  Then, in this order:
 *   1. db > dialog_db: if n_background > 0 it goes to 0 and the open section closes; ++n_dialog; if n_dialog >= min_run
 *      and no section is open, a dialog section opens AT THIS HOP (the first min_run - 1 hops of a run are not part of it)
 *   2. else, (db > bridge_db or level < silence_db) and n_dialog >= min_run: the hop belongs to the open section, the
 *      counters do not move
 *   3. else, db < background_db: the mirror image of 1 for background
 *   4. else: both counters go to 0 and the open section closes.
 * A closed section is {kind, first_hop, end_hop} with end_hop exclusive, in hops since the state's reset (samples: * 1024).
 * bsrnn_sections_scan consumes n_hops pairs of act_host [n_hops][2] (one row of a downloaded act_dev), with flush != 0 then
 * closes an open section behind the last hop, writes the first `cap` sections the call closed to `out` and their number to
 * *n_out - which may exceed cap: the state advances over all hops whatever cap is, so a caller sizes with cap = 0 on a copy
 * of its state and repeats.  Feeding a stream's hops in any split gives the sections of one call.  rule NULL: the defaults.
 * BSRNN_EARG: a null state or n_out, a negative n_hops or cap, min_run < 1, act_host NULL with n_hops > 0, out NULL with
 * cap > 0.  These three functions need no context and no GPU. */
#define BSRNN_ACT_RATIO 0
#define BSRNN_ACT_LEVEL 1
#define BSRNN_SECTION_NONE       0
#define BSRNN_SECTION_DIALOG     1
#define BSRNN_SECTION_BACKGROUND 2
typedef struct bsrnn_section_rule {
    double  dialog_db, bridge_db, background_db, silence_db;
    double  level_floor, floor_db;
    int32_t min_run;
} bsrnn_section_rule;
typedef struct bsrnn_section_state {
    int64_t n_dialog, n_background;
    int32_t open_kind;               /* BSRNN_SECTION_* */
    int64_t open_hop;                /* first hop of the open section */
    int64_t hop;                     /* hops consumed so far */
} bsrnn_section_state;
typedef struct bsrnn_section {
    int32_t kind;                    /* BSRNN_SECTION_DIALOG or _BACKGROUND */
    int64_t first_hop, end_hop;
} bsrnn_section;
int  bsrnn_hop_activity(bsrnn_ctx* ctx, const float* mix_dev, int64_t mix_stride, const float* est_dev, int64_t est_stride,
                        const int32_t* hops_host, int32_t R, int32_t Hmax, double* act_dev, void* stream);
void bsrnn_section_rule_default(bsrnn_section_rule* rule);
void bsrnn_section_state_reset(bsrnn_section_state* state);
int  bsrnn_sections_scan(const bsrnn_section_rule* rule, bsrnn_section_state* state, const double* act_host, int64_t n_hops,
                         int32_t flush, bsrnn_section* out, int64_t cap, int64_t* n_out);

/* ---- re-mix: the mixtures and targets of an optimizer step in one launch ------------------
 * The reference's MixDataSet (m_dataset.py:141-180) makes a training item from one dialog and four backgrounds: every
 * background is padded or cut to the item's length at a random place and scaled, and the mixture is
 * dialog + sum(backgrounds).  bsrnn_remix_ragged forms the items of a whole optimizer step from sources that stay on the
 * device, straight into the padded [rows][width] buffers bsrnn_stft_ragged ... bsrnn_train_loss_ragged take.  The draws
 * (which sources, where, how loud) are the host's; the call is the arithmetic.
 *
 * Row r owns terms [first_term, first_term + n_terms) of terms_host, n_terms >= 1: the first is the target (the dialog),
 * the others the backgrounds, in order.  The value of term t at output sample i is
 *     v_t(i) = src[i - at] * gain   if 0 <= i - at < len,   else +0
 * - the product is one fp32 multiply; at > 0 is the reference's left padding, at < 0 its cut; src is read nowhere else and
 * may be null only if len == 0.  For 0 <= i < rows_host[r].n
 *     target_dev[r * target_stride + i] = v_0(i)
 *     mix_dev[r * mix_stride + i]       = v_0(i) + ((((+0 + v_1(i)) + v_2(i)) + ...)
 * every + one fp32 addition in that order and no product fused into an addition: Python's `dialog + sum(backgrounds)`, bit
 * for bit (torch multiplies a float32 tensor by a Python float as x * float32(g); 0 + b and d + 0 turn -0 into +0, so a
 * target of -0 without background gives mix +0 and target -0; a gain of 1.0f is the identity, which is what the
 * reference's dialog carries, its `dialog *= scale_dialog` being commented out).  inf and NaN pass through by position.
 * For n <= i < width both outputs are +0 - callers need no memset - and nothing is written behind width in a row.  A
 * row's bits depend on its terms alone, not on the other rows, on alignment or on the strides.  Terms may share sources
 * (a mono source serves both rows of a clip through one pointer) and rows may share terms.
 * Valid: R >= 1, n_terms >= 1, 0 <= n <= width <= both strides (n = 0 is a legal all-zero row; width and the strides at
 * most 2^40, (R - 1) * stride at most 2^60), every row's term range inside [0, n_terms), 0 <= len <= 2^40, |at| <= 2^40.
 * Everything else is refused with BSRNN_EARG and a sentence that names the row or term, before the device is touched -
 * null tables, null outputs and a null ctx too, on a host-only context in front of its BSRNN_ESTATE.  Outputs that
 * overlap each other or any source are UNDEFINED and not checked (a source is any device memory).  One launch of grid
 * (ceil(width / BSRNN_REMIX_TILE), R); the tables travel with the call and are the caller's again at return; asynchronous
 * on `stream`; needs no committed weights and allocates nothing once a call of its table size has been made. */
#define BSRNN_REMIX_TILE 2048        /* consecutive outputs of a row one workgroup forms */
typedef struct bsrnn_remix_term { const float* src; int64_t len; int64_t at; float gain; int32_t pad_; } bsrnn_remix_term;
typedef struct bsrnn_remix_row  { int64_t n; int32_t first_term; int32_t n_terms; } bsrnn_remix_row;
int  bsrnn_remix_ragged(bsrnn_ctx* ctx, const bsrnn_remix_row* rows_host, int32_t R, const bsrnn_remix_term* terms_host, int32_t n_terms,
                        float* mix_dev, int64_t mix_stride, float* target_dev, int64_t target_stride, int64_t width, void* stream);

/* ---- measurement support ---------------------------------------------------------------
 * bsrnn_set_profiling(ctx, mask): bit i of `mask` brackets stage i of every compute call with
 * hipEvents on the call's stream (mask < 0 = all stages, 0 = off; each bracket costs ~10 us of
 * stream time, so time-critical runs enable only the stage they report);
 * bsrnn_stage_times() synchronises on the last call and returns per-stage elapsed
 * milliseconds (accumulated since the last reset) and launch counts.  Every model entry point records its stages,
 * bsrnn_dual_path included (band_lstm, band_fc, time_lstm, time_fc).  Stage names:
 * bsrnn_stage_name(i).  Used by bench.py for the live roofline figure. */
int         bsrnn_set_profiling(bsrnn_ctx* ctx, int32_t on);
int         bsrnn_stage_count(void);
const char* bsrnn_stage_name(int32_t i);
int         bsrnn_stage_times(bsrnn_ctx* ctx, double* ms_out, int64_t* launches_out, int32_t reset);

/* ---- device memory helpers for hosts without a HIP binding (the plugin, C tests) -------- */
int  bsrnn_dev_alloc(bsrnn_ctx* ctx, int64_t nbytes, void** out);
int  bsrnn_dev_free(bsrnn_ctx* ctx, void* p);
int  bsrnn_copy_h2d(bsrnn_ctx* ctx, void* dst_dev, const void* src_host, int64_t nbytes);
int  bsrnn_copy_d2h(bsrnn_ctx* ctx, void* dst_host, const void* src_dev, int64_t nbytes);
int  bsrnn_sync(bsrnn_ctx* ctx, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BSRNN_HIP_H */
