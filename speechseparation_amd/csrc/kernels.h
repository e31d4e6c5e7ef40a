// Internal launcher interface between the host units (api*.hip) and the gfx950 kernels.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "descriptors.h"   // GemmJob, ChainDesc and the constants the host packs against (HIP-free)
#include "stream_rows_host.h"   // RowSet: the rows a streaming rows call means, by value (HIP-free)
#include "resample_bank_host.h" // BankRow: what a resampler bank's kernel knows of a row, by value (HIP-free)
#include "train_ragged_host.h"  // TrainClip: what the ragged training loss kernels know of a clip (HIP-free)
#include "pool_host.h"          // PoolEntry: what the native session pool's copy kernels know of a row (HIP-free)
#include "convolve_host.h"      // ConvRow: what the FIR convolution's kernels know of a row (HIP-free)
#include "convolve_stream_host.h"   // FirStreamRow: what the streaming FIR kernel knows of a row in one call (HIP-free)
#include "metrics_host.h"       // MetricClip, METRIC_TIME_Q: what the metric kernels and their host tail agree on (HIP-free)
#include "remix_host.h"         // RemixRow, RemixTerm: what the re-mix kernel knows of a row and of a term (HIP-free)
#include "critic_host.h"        // CriticLayout: tiles, K slabs and reduction chunks of the critic's convolution (HIP-free)
#include "critic_score_host.h"  // CscPlan: the committed critic's weight image, K slabs and workspace (HIP-free)
#include "critic_grad_host.h"   // CgdPlan: the committed critic's dx image, tiles and workspace (HIP-free)
#include "critic_ragged_host.h" // CrgPlan: the committed critic on a padded batch, its tables and workspace (HIP-free)
#include "critic_spectrum_host.h"   // CsSlab: the rows x frames one launch pair of the critic's 4096-point analysis owns (HIP-free)

namespace bsrnn {

// ------------------------------------------------------------------ grouped linear layers (GemmJob: descriptors.h)
enum GemmEpilogue {
    EPI_LINEAR = 0,      // y = acc + b
    EPI_LEAKY = 1,       // y = leaky_relu(acc + b, 0.01)
    EPI_RES = 2,         // y = acc + b + R                         (NormRNNResidual, bsrnn.py:84-86)
    EPI_MASK = 3         // mask = acc + b + R ; y = Mul * mask      (bsrnn.py:425, :441)
};

struct GemmLaunch {
    const GemmJob* jobs;     // device array
    const int2* tiles;       // device array [n_tiles]: (job index, column-tile index inside the job)
    int n_tiles;
    int tile_n;              // column-tile width of this launch: 64 or 128
    int mchunk;              // m-tiles per XCD-pinned chunk (filled in by launch_gemm)
    const float* X; int ldx;
    float* Y; int ldy;
    const float* R; int ldr;
    const float* Mul; int ldm;
    float* tap; int ldt;     // optional mask tap (EPI_MASK), may be null
    int M;
    int epilogue;
    int* range_flag;                   // fp16x2: set to 1 when an operand exceeded the fp16 range (may be null)
};
void launch_gemm(const GemmLaunch& g, hipStream_t stream);
// Small-M path (gemv.hip): the same launch on the vector ALU in exact fp32, for calls of a few frame rows (the one-frame
// streaming step: C rows).  api.hip uses it for every per-layer launch of a call with C * L <= GEMV_MAX_FRAME_ROWS (descriptors.h).
void launch_gemv(const GemmLaunch& g, hipStream_t stream);
// How the Linear layers are evaluated: GemmMode (descriptors.h), from the environment BSRNN_GEMM, read once per process.
int gemm_mode();
void set_force_f32(bool on);
bool force_f32();
constexpr int GEMM_BM = 128;

// ------------------------------------------------------------------ fused per-band MLP chains (mlp_chain.hip; ChainDesc: descriptors.h)
struct ChainLaunch {
    const ChainDesc* desc;   // device array
    const int2* tasks;       // device array [n_tasks]: (descriptor index, first frame row) of every workgroup, in dispatch order
    int n_tasks;             //   (built per M by build_chain_tasks(), plan_host.h: descriptor after descriptor, all row blocks of a band together)
    int M;
    const float* Xin; int ldx;       // SPLIT: spectrum rows; MASK: Z rows
    float* P; int ldp;               // SPLIT: written (bandFCs_pre output = the mask's residual); MASK: read
    float* Z; int ldz;               // SPLIT: written
    const float* Xmul; int ldm;      // MASK: the spectrum the mask multiplies
    float* Y; int ldy;               // MASK: x * mask
    float* tap; int ldt;             // MASK: the mask itself (optional)
    int* range_flag;
    unsigned long long* dbg;         // measurement only (CHAIN_TRACE builds of tools/chain_bench.hip): per-wave phase stamps
    // MASK chain launched BESIDE the time-axis launch that produces its input (api.hip, overlapped dual path): every workgroup first
    // waits until the frames of its rows have left that launch (OvlConsumer below); null = the input is complete at launch
    const int* ovl_prog; int ovl_T, ovl_K, ovl_spin, ovl_base, ovl_wg_shift;
};
void launch_mlp_chain(const ChainLaunch& g, int chain, hipStream_t stream);

// ------------------------------------------------------------------ overlapped dual path (api.hip: run_overlapped)
// A time-axis launch is causal and the launch behind it (the next band block, the mask chain) works frame by frame, so that launch is
// started on a second stream BESIDE the time-axis launch - on the 64 CUs its 192 workgroups leave idle and on every CU one of them
// frees - and each of its workgroups waits until the frames of its own rows have left the time-axis launch:
//   producer (time_lstm_h2w_kernel): resident[0] += 1 per workgroup at its start (the consumer launch is gated on ALL of them being
//       resident, so a waiting consumer can never keep a producer off the chip); every output row is stored write-through (sc1);
//       prog[wg] += 1 for every finished group of four steps, by the last of the four storing waves behind each one's vmcnt(0);
//   consumer: one lane polls prog[] of the time workgroups that own its rows (relaxed agent-scope loads, bounded), one agent-scope
//       acquire, workgroup barrier, then plain loads (cdna_hip_programming.md, Guideline 16).  A wait that expires is REPORTED (range
//       flag value 5: api.hip runs the call again launch after launch and stops overlapping), never computed with.
// All words are zeroed in stream order before the producers of a call start; nothing travels by value that changes from call to call.
// Progress words carry the CALL'S EPOCH in their upper bits (api.hip counts overlapped calls per context): prog[wg] = epoch << 12 | groups done,
// raised with an atomic max; the resident counters only ever grow and a gate waits for the context's running total.  So nothing is zeroed per
// call and nothing orders the consumer's stream behind the producer's except the words themselves (an overlapped call is never captured into
// a graph - api.hip - so by-value epochs cannot go stale; every 2^18 calls the host drains the device and starts the epochs again).
struct OvlProducer { int* resident; int* prog; int base; };                          // base = epoch << OVL_EPOCH_SHIFT
struct OvlConsumer { const int* prog; int T; int spin_limit; const int* order; int base; int wg_shift; };   // spin_limit: 100 MHz ticks a wait may last; wg_shift: log2 of the producer's sequences per workgroup
// OVL_EPOCH_SHIFT: descriptors.h.  order (band launch): dispatch ordinal -> tile of 16 sequences, by the time its frames are ready
constexpr int OVL_SPIN_LIMIT = 20000000;       // 100 MHz ticks (s_memrealtime) before a wait gives up: 200 ms - a healthy wait lasts as long as a
                                               // time-axis launch (0.1 ... a few ms); under a tool that serialises kernels (rocprofv3 --pmc) the
                                               // producer never runs beside the consumer: the call falls back after this long, once per context
void launch_ovl_gate(const int* resident, int target, int* range_flag, int spin_limit, hipStream_t stream);
int device_cus();                                  // CUs of the current device (256 on MI355X), read once
#if defined(__HIPCC__)
// frame rows m_first .. m_last (m = batch row * T + frame) of bands k_first .. k_last: wait until every time-axis workgroup that owns one
// of those sequences (n = batch row * K + band, 1 << wg_shift per workgroup) has published the groups that cover the frames.  ONE lane calls this.
__device__ __forceinline__ bool ovl_wait_rows(const int* prog, int m_first, int m_last, int T, int K, int k_first, int k_last, int limit, int base, int wg_shift)
{
    typedef const int __attribute__((address_space(1)))* gci;
    const gci pg = (gci)prog;
    const int r_a = m_first / T, r_b = m_last / T;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int r = r_a; r <= r_b; ++r) {
        const int t_last = r < r_b ? T - 1 : m_last - r * T;
        const int need = base + (t_last >> 2) + 1;
        for (int wg = (r * K + k_first) >> wg_shift; wg <= (r * K + k_last) >> wg_shift; ++wg)
            while (__hip_atomic_load(pg + wg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
                __builtin_amdgcn_s_sleep(16);
                if (__builtin_amdgcn_s_memrealtime() - t0 > (unsigned long long)limit) return false;
            }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");          // this CU's L1 holds nothing older than the poll
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // ... once the invalidate has completed (the caller's barrier follows)
    return true;
}
#endif

// ------------------------------------------------------------------ dual-path LSTM kernels
// Band-axis BLSTM layer (both directions in one launch): N sequences of length L.
//   xin  [N][L][IN]           IN = 64 (layer 0, fc_in folded into W_ih) or 128 (layer 1)
//   hout [N][L][128]          forward half at [0,64), backward half at [64,128)
//        In the fp16x2 mode the IN = 64 launch (layer 0) writes its output as the two fp16 planes it already has for its own
//        recurrence - per (sequence, step): [piece 0: 128 halves][piece 1: 128 halves], the same 512 bytes - and the IN = 128
//        launch (layer 1) expects exactly that as xin: the pair is always launched back to back on the same buffer (api.hip);
//        the exact-fp32 kernels (BSRNN_LSTM=f32, range-guard re-run) exchange plain fp32.
//   wpk  packed [2 dir][4 wave][(IN+64)/4 step][4 gate][64 lane], bias [2][256]
//   wpk16 (LSTM_FP16X2): the same matrix as two fp16 pieces in the f16 MFMA's B-operand order,
//         [2 dir][4 wave][(IN+64)/32 blk][4 gate][2 piece][64 lane][8]
//   f32: the exact-fp32 kernels (BSRNN_LSTM=f32, range-guard re-run), else fp16x2
void launch_band_lstm(const float* xin, float* hout, const float* wpk, const void* wpk16, const float* bias,
                      int N, int L, int IN, int* range_flag, hipStream_t stream, bool f32);
// The block's fc in parts (BSRNN_BAND_FC): with fc16 / fcb the pair launch below writes to hb1, instead of h, the two directions' SHARES
// of fc(h): hb1[n][t][dir * 64 + f] = sum_k W_fc[f][dir * 64 + k] h_dir[n][t][k] (+ b[f] in the forward half); the time-axis launch
// adds the halves and the residual (`part` of launch_time_lstm), so the block's fc launch disappears.
// Both layers of a band block in one launch (lstm.hip::band_pair_h2_kernel, fp16x2 only): flags = 2 ints per tile of 16 sequences, zero
// before the first launch and otherwise only touched by these launches (one or two tiles per workgroup: the same flags, counted alike).
void launch_band_pair(const float* z, float* hb0, float* hb1, const void* w0pk16, const float* bias0, const void* w1pk16, const float* bias1,
                      int N, int L, int* range_flag, hipStream_t stream, const void* fc16, const float* fcb, int* flags,
                      const OvlConsumer* ovl = nullptr, int* zero_words = nullptr, int zero_n = 0, hipEvent_t done = nullptr,   // zero_words: progress words to clear (overlapped dual path)
                      int tiles = 1);                                     // tiles of 16 sequences per workgroup, 1 or 2 (plan_host.h::band_pair_tiles)
// The whole band-axis block (both layers, both directions, fc + residual) of a few sequences in one workgroup: the streaming
// step's N = C frame rows.  w0pk16 / w1pk16 / bias0 / bias1 are launch_band_lstm's arguments of the two layers; fc16 the block's
// fc (128 -> 64) as fp16x2 B fragments [4 tile][4 blk][2 piece][64 lane][8], fcb its bias.  zout = fc(h1) + b + zin.
// fp16x2 only; 1 <= N <= 8 sequences of 1 <= L <= BS_MAXL steps (api.hip decides when a call takes it).
void launch_band_block_small(const float* zin, float* zout, const void* w0pk16, const float* bias0, const void* w1pk16, const float* bias1,
                             const void* fc16, const float* fcb, int N, int L, int* range_flag, hipStream_t stream);
// How the recurrent layers evaluate their gate products: LstmMode (descriptors.h), from the environment BSRNN_LSTM, read once.
int lstm_mode();
// Time-axis LSTM, both layers pipelined in one launch, causal with state carry.
//   zin/hout [R][T][K][64]; sequences n = r*K + k;  wpk packed [2 layer][4 wave][128 k][64 lane]
//   state_in/out [2 (h,c)][2 layer][R*K][64] or null
//   wpk16 (LSTM_FP16X2): two fp16 pieces in B-operand order, [2 layer][4 wave][4 blk][4 gate][2 piece][64 lane][8]
//   f32: the exact-fp32 kernel (time_lstm_kernel; wpk), else the fp16x2 kernels (wpk16)
//   seqs: sequences per workgroup of the fp16x2 launch: 4 (time_lstm_h2w_kernel), or 8 (time_lstm_h2w8_kernel, with fc16 / fcb only)
//   fc16 / fcb (fp16x2, optional): the block's trailing fc (bsrnn.py:84) as two fp16 pieces in B-operand order,
//         [4 wave][2 blk][2 piece][64 lane][8], and its bias [64].  When both are given, the launch writes the BLOCK's output
//         fc(h1) + b + zin to hout (h1 never leaves the chip); otherwise hout = h1.
//   part (with fc16 / fcb only, optional) [R][T][K][2][64]: the block's input is zin + part[.., 0, :] + part[.., 1, :] instead of zin
//         (the shares of the preceding band block's fc, see launch_band_lstm); hout must then be a different buffer than zin.
void launch_time_lstm(const float* zin, float* hout, const float* wpk, const void* wpk16, const float* bias,
                      const float* state_in, float* state_out, int R, int T, int K, int* range_flag, hipStream_t stream,
                      bool f32, int seqs, const void* fc16 = nullptr, const float* fcb = nullptr, const float* part = nullptr,
                      const OvlProducer* ovl = nullptr,    // ovl: with fc16 / fcb / part only (the fused launch of the parts flow)
                      const int* row_frames = nullptr);
//   row_frames (optional) [R] on the device: the ragged instantiations (bsrnn_stream_process_hops) - state_out holds the state of row
//         r's sequences after step row_frames[r] - 1 instead of after step T - 1 (anything for a row at 0); all T steps are still run
//         and published, and hout is unspecified but finite from a row's count on

// ------------------------------------------------------------------ training step, part 1: recurrent layers (lstm_train.hip)
// One nn.LSTM layer (bsrnn.py:66-72) with ndir directions over N sequences of L steps, exact fp32; weights in torch layout
// (w_ih [ndir][256][IN], w_hh [ndir][256][64], bias [ndir][256] = b_ih + b_hh), zero initial state.
//   forward:  x [N][L][IN] -> h [N][L][ndir 64], gates [N][L][ndir][256] (after the non-linearities), cells [N][L][ndir][64]
//   backward: dh [N][L][ndir 64] -> dx [N][L][IN] (or null), dw_ih, dw_hh, db (= db_ih = db_hh) in the weights' layouts;
//             dg [N][L][ndir][256] and scratch [lstm_train_scratch_floats] are workspace
constexpr int LSTM_TRAIN_CHUNKS = 64;        // row chunks of the weight-gradient reductions (summed in a fixed order): ~512 rows each
constexpr int LSTM_TRAIN_MAX_CHUNKS = 256;   // ... more, up to this, when the gradient has only a few 64 x 64 tiles
// generic fp32 products of the training step (train_ops.hip): C (+)= A op(B) (+ bias) (LeakyReLU); out = A^T B with an optional
// step shift of B's rows (h_prev); column sums.  Scratch = partial sums of the row chunks.
// a group of products in one launch (the same layer of all bands); passed by value in the kernel arguments
constexpr int GEMM_GROUP = 12;
struct TrainGemmJob {
    const float* A; const float* B; float* C; const float* bias;
    int lda, ldb, ldc;
    int M, N, K;
    int tiles_x, tiles_y, rpc;      // filled in by the launchers
};
struct TrainGemmGroup { TrainGemmJob j[GEMM_GROUP]; int first[GEMM_GROUP + 1]; int count; };
struct ReduceJob { const float* part; float* out1; float* out2; int n1, n2, chunks; };
struct ReduceGroup { ReduceJob j[GEMM_GROUP]; int first[GEMM_GROUP + 1]; int count; };
void launch_sgemm_group(TrainGemmGroup& g, int trans_b, int accumulate, int leaky, hipStream_t stream);      // C_i (+)= A_i op(B_i) (+ bias_i)
size_t tn_group_scratch_floats(const TrainGemmGroup& g);
void launch_sgemm_tn_group(const TrainGemmGroup& g, float* scratch, int L, int shift, hipStream_t stream);   // C_i = A_i^T B_i, bias_i = column sums of A_i
size_t sgemm_tn_scratch_floats(int M, int N1, int N2);
void train_reduction_layout(int M, int N1, int N2, int out[2]);           // {chunks, rows per chunk} of A^T B over M rows, C [N1][N2]
size_t colsum_scratch_floats(int M, int cols);
void launch_sgemm(const float* A, int lda, const float* B, int ldb, int trans_b, float* C, int ldc, int M, int N, int K,
                  int accumulate, const float* bias, int leaky, hipStream_t stream);
void launch_sgemm_tn(const float* A, int lda, const float* B, int ldb, float* out, float* colsum, float* scratch, int M, int N1, int N2,
                     int L, int shift, hipStream_t stream);
void launch_colsum(const float* A, int lda, float* out, float* scratch, int M, int cols, hipStream_t stream);
// one AdamW update of n parameters (torch.optim.AdamW semantics; bc1 = 1 - beta1^t, bc2s = sqrt(1 - beta2^t))
void launch_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, double b1, double b2, float eps, float wd,
                  float bc1, float bc2s, hipStream_t stream);
// the same update for up to ADAM_GROUP tensors in one launch; everything travels by value in the kernel arguments
constexpr int ADAM_GROUP = 80;
struct AdamGroup {
    float* p[ADAM_GROUP]; const float* g[ADAM_GROUP]; float* m[ADAM_GROUP]; float* v[ADAM_GROUP];
    int n[ADAM_GROUP];                  // elements per tensor (< 2^31)
    int first_block[ADAM_GROUP + 1];    // prefix sums of ceil(n / 1024)
    int count;
};
// state != nullptr: {lr, bc1, bc2s, step(int32)} in device memory override the by-value arguments (launch_adamw_tick advances it)
void launch_adamw_group(const AdamGroup& a, float lr, double b1, double b2, float eps, float wd, float bc1, float bc2s, hipStream_t stream,
                        const float* state = nullptr);
void launch_adamw_tick(float* state, double b1, double b2, hipStream_t stream);
// nn.Linear (+ LeakyReLU(0.01)) for a group of layers that share the row count M (the same layer of all bands):
struct LinearJob {
    const float* x; int ldx;        // [M][K], row stride ldx
    const float* w; const float* b; // W [N][K] (torch layout), b [N]
    float* y; int ldy;              // forward output / backward input (read when leaky)
    const float* dy; int lddy;      // backward: gradient of y
    float* dx; int lddx;            // backward: gradient of x (null: not wanted)
    float* dw; float* db;           // backward: gradients of W and b
    int K, N;
};
void launch_linear_group_forward(const LinearJob* jobs, int n, int M, int leaky, hipStream_t stream);
size_t linear_group_scratch_floats(const LinearJob* jobs, int n, int M, int leaky);
void launch_linear_group_backward(const LinearJob* jobs, int n, int M, int leaky, float* scratch, hipStream_t stream);
// nn.Linear (+ LeakyReLU(0.01)): y = act(x W^T + b), W [N][K]; backward: dx (may be null), dW, db from dy (and y when leaky)
size_t linear_train_scratch_floats(int M, int K, int N, int leaky);
void launch_linear_train_forward(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int M, int K, int N,
                                 int leaky, hipStream_t stream);
void launch_linear_train_backward(const float* x, int ldx, const float* w, const float* y, int ldy, const float* dy, int lddy,
                                  float* dx, int lddx, float* dw, float* db, float* scratch, int M, int K, int N, int leaky,
                                  hipStream_t stream);
size_t lstm_train_scratch_floats(int N, int L, int IN, int ndir);
void launch_lstm_train_forward(const float* x, const float* w_ih, const float* w_hh, const float* bias, float* h, float* gates,
                               float* cells, int N, int L, int IN, int ndir, hipStream_t stream);
void launch_lstm_train_backward(const float* x, const float* h, const float* gates, const float* cells, const float* dh,
                                const float* w_ih, const float* w_hh, float* dg, float* scratch, float* dx, float* dw_ih,
                                float* dw_hh, float* db, int N, int L, int IN, int ndir, hipStream_t stream);

// ------------------------------------------------------------------ STFT / iSTFT / layout
struct FftTables {           // device tables, built once per context (double precision on host)
    const float2* tw1024;    // exp(-2 pi i k / 1024), k < 1024
    const float2* tw2048;    // exp(-2 pi i k / 2048), k <= 1024
    const float* hann;       // periodic Hann(2048)
    const float* inv_env;    // 1 / (w^2[i] + w^2[i+1024]), i < 1024   (torch.istft envelope)
    const float* inv_wsum;   // 1 / (w[i] + w[i+1024]),   i < 1024   (infer-streaming.py:145)
    // band-padded spectrum layout: bin k's (re, im) sit at columns colmap[k], colmap[k]+1 of a row of ld floats;
    // every band starts at a multiple of 4 floats so that the first Linear layer can use 16-byte loads
    const int* colmap;       // [1025]
    int ld;
};
// wave [R][n] -> X frame-major [R*T][ld] (re/im interleaved, band-padded columns), reflect padding, Hann.
void launch_stft(const FftTables& tb, const float* wave, float* X, int R, int64_t n, int T, hipStream_t s);
// Y frame-major [R*T][ld] -> wave_out [R][(T-1)*1024]: inverse real FFT, synthesis window, overlap-add / envelope, fused
void launch_istft(const FftTables& tb, const float* Y, float* out, int R, int T, hipStream_t s);
// The same pair for frames [ta, te) of the clip alone (bsrnn_separate_long; fft.hip), segment-local rows X / Y [R*(te-ta)][ld]:
//   analysis: src = the clip (stride = n, base = 0) or a staged window of it that starts at clip sample `base`, rows `stride` floats apart;
//             reflection is at the clip's ends
//   synthesis: writes the hops the segment completes, [max(ta-1, 0), te-1), to out (its first hop of row 0; rows out_stride floats apart);
//             carry_in [R][1024] = the windowed second half of frame ta-1 as the previous segment's launch left it (null: ta = 0),
//             carry_out [R][1024] = that of frame te-1 (another buffer than carry_in)
void launch_stft_segment(const FftTables& tb, const float* src, int64_t stride, int64_t base, float* X, int R, int64_t n, int ta, int te, hipStream_t s);
void launch_istft_segment(const FftTables& tb, const float* Y, float* out, int64_t out_stride, const float* carry_in, float* carry_out, int R, int L,
                          hipStream_t s);
// The same pair for rows of different lengths (bsrnn_separate_ragged; fft.hip): row r holds lens[r] samples (device int64) at wave + r * stride
// and T_r = 1 + lens[r] / 1024 frames of the rectangle X / Y [R*Tmax][ld]; its frames t >= T_r are written as zero rows of X, its hops
// b >= T_r - 1 as zeros of out (rows out_stride floats apart, Tmax - 1 hops each)
void launch_stft_ragged(const FftTables& tb, const float* wave, int64_t stride, const int64_t* lens, float* X, int R, int Tmax, hipStream_t s);
void launch_istft_ragged(const FftTables& tb, const float* Y, float* out, int64_t out_stride, const int64_t* lens, int R, int Tmax, hipStream_t s);
// Both at once (bsrnn_separate_long_ragged; fft.hip): frames [ta, te) of a ragged batch, segment-local rows X / Y [Ri*(te-ta)][ld] for the Ri
// rows of the segment's alive prefix (plan_host.h, ragged_long_plan).  The analysis runs on those Ri rows (frames t >= T_r as zero rows); the
// synthesis on all R rows of the call - out, carry_in, carry_out as launch_istft_segment's, hops that are not a row's own stored as zeros,
// carry_out[r] zeros for a row without a frame te.  launch_long_compact: the state ([4][2][R_old*K][64] -> [4][2][R_new*K][64]) and the carry
// of the first R_new rows from one carry set into the other when the prefix shrinks.
void launch_stft_ragged_segment(const FftTables& tb, const float* wave, int64_t stride, const int64_t* lens, float* X, int Ri, int ta, int te, hipStream_t s);
void launch_istft_ragged_segment(const FftTables& tb, const float* Y, float* out, int64_t out_stride, const int64_t* lens, const float* carry_in,
                                 float* carry_out, int R, int Ri, int ta, int te, hipStream_t s);
void launch_long_compact(const float* state_src, float* state_dst, const float* carry_src, float* carry_dst, int R_old, int R_new, int K, hipStream_t s);
// gradient of launch_istft's output w.r.t. its input (training step): dwave [R][(T-1)*1024] -> dY frame-major [R*T][ld];
// scratch [R][(T-1)*1024]
void launch_istft_backward(const FftTables& tb, const float* dwave, float* scratch, float* dY, int R, int T, hipStream_t s);
// the same for launch_istft_ragged's output, row by row: dwave, scratch [R][(Tmax-1)*1024] (row r read / written below n_est_r only) ->
// dY frame-major [R*Tmax][ld], zero rows for frames t >= T_r
void launch_istft_ragged_backward(const FftTables& tb, const float* dwave, float* scratch, float* dY, const int64_t* lens, int R, int Tmax,
                                  hipStream_t s);
// [C][2050][T] (reference layout) <-> [C*T][ld] (band-padded)
void launch_to_frame_major(const FftTables& tb, const float* x, float* xf, int C, int T, hipStream_t s);
void launch_from_frame_major(const FftTables& tb, const float* yf, float* y, int C, int T, hipStream_t s);
// Which rows of a streaming call take how many of its hops: all of them every hop (the plain calls), only the rows of a set
// (bsrnn_stream_process_rows), or every row its own count (bsrnn_stream_process_hops).  Set and counts travel by value in the kernel
// arguments (stream_rows_host.h); mix_rows, if not null, holds one wet / dry value per row [C] on the device and replaces `mix`
// (never with ALL).  The launchers below pick the kernel instantiation by `kind`.
struct StreamRows {
    enum Kind { ALL, HELD, HOPS } kind = ALL;
    RowSet active;                     // HELD
    RowHops hops;                      // HOPS (the block launches only: a one-hop call never meets mixed counts)
    const float* mix_rows = nullptr;
};
// streaming DSP, one frame per row (infer-streaming.py:116-145).  What a step carries to the next one is read from one buffer and
// written to another (the stream object alternates two sets): a step can be run again from its unchanged starting point.
//   analysis: buf_out [C][2048] = [buf_in[:, 1024:], chunk [C][1024]]; X [C][ld] = rfft(buf_out * hann)
//   synthesis: s = irfft(mix(Y, X)); out = (s[0:1024] + prev_in[1024:2048]) * inv_wsum; prev_out = s
// A held row (HELD, not in the set): buf_out / prev_out = buf_in / prev_in, zero rows in X, zeros in out, chunk unread - and, in the
// synthesis, its LSTM state copied from state_in to state_out [4][2][C*K][64], so that launch follows the model's.  Active rows: the
// bits of the plain launches.
void launch_stream_analysis(const FftTables& tb, const float* buf_in, float* buf_out, const float* chunk, float* X, int C, const StreamRows& rows,
                            hipStream_t s);
void launch_stream_synthesis(const FftTables& tb, const float* Y, const float* X, float mix, const float* prev_in, float* prev_out, float* out,
                             const float* state_in, float* state_out, int C, int K, const StreamRows& rows, hipStream_t s);
// The same for L consecutive hops per row in one launch each (bsrnn_stream_process): chunk / out [C][L*1024], X / Y frame-major
// [C*L][ld] (row c*L + l).  buf_out = the last 2048 samples of buf_in ++ chunk, prev_out = the last synthesis frame.
// HOPS: row r with n = row_hops_of(hops, r) - frames / hops below n as the plain launches give them, zero rows of X / zeros of out from
// n on, chunk unread from n * 1024 on, buf_out / prev_out the carry after n hops; n = 0 is a held row.  The analysis writes
// row_frames[r] = n ([C] on the device) for the call's time-axis launches (launch_time_lstm).
void launch_stream_block_analysis(const FftTables& tb, const float* buf_in, float* buf_out, const float* chunk, float* X, int C, int L,
                                  const StreamRows& rows, int* row_frames, hipStream_t s);
void launch_stream_block_synthesis(const FftTables& tb, const float* Y, const float* X, float mix, const float* prev_in, float* prev_out, float* out,
                                   const float* state_in, float* state_out, int C, int K, int L, const StreamRows& rows, hipStream_t s);
// zeroes buf, prev and state of the rows in `rows` of one carry set, in one launch (bsrnn_stream_reset_rows)
void launch_stream_reset_rows(float* buf, float* prev, float* state, int C, int K, const RowSet& rows, hipStream_t s);

// Long FIR convolution of ragged rows (bsrnn_convolve_ragged; fft.hip, the plan: convolve_host.h).  launch_fir_taps: the image
// H [P][CONV_LD] of one filter from its k taps on the device.  launch_fir_group: rows [row0, row0 + n_rows) of the table `rows` (on the
// device) - analysis into X, multiply-accumulate into Y, synthesis into out; max_nx / max_nb the largest frame / block count among them
// (copied rows: no frames, their pieces of 1024 samples as blocks).  in / out are the call's, rows in_stride / out_stride apart.
void launch_fir_taps(const FftTables& tb, const float* taps, int k, float* H, hipStream_t s);
void launch_fir_group(const FftTables& tb, const ConvRow* rows, int row0, int n_rows, int max_nx, int max_nb, const float* in, int64_t in_stride,
                      float* out, int64_t out_stride, float* X, float* Y, hipStream_t s);
// The streaming form (bsrnn_fir_stream_*; the plan: convolve_stream_host.h): one launch, one workgroup per row of the table `rows` [C] (on
// the device).  ring [C][ring_stride] floats (a row's P slots of CONV_LD at its start), state [C][FIR_STREAM_ROW_FLOATS] (the previous
// 1024 inputs, then the FIFO).  in / out may be null when no row reads / writes.
void launch_fir_stream(const FftTables& tb, const FirStreamRow* rows, int C, const float* in, int64_t in_stride, float* out, int64_t out_stride,
                       float* ring, int64_t ring_stride, float* state, hipStream_t s);

// ------------------------------------------------------------------ validation metrics (metrics.hip)
// One family for the three evaluate calls: per-workgroup partial sums in double, which the host adds (metrics_host.h: METRIC_TIME_Q sums
// per row - s^2, (x-s)^2, x*s, x^2, |x-s|, m^2, (m-x)^2 - and MetricClip).  A batch is rows and clips of their own lengths: lens [R] the
// rows' lengths on the device (T_r = 1 + lens[r] / 1024 frames inside the rectangle R x Tmax, n_est_r = (T_r - 1) * 1024 samples), est rows
// out_stride floats apart, speech and mix rows wave_stride floats apart.  bsrnn_evaluate's rectangle [R][n] is the batch of one clip {0, R, n}
// with R equal lengths, wave_stride = n and out_stride = n_est.  Every slot of every partial array is written.
// chunks = metric_time_chunks((Tmax - 1) * 1024).
int metric_time_chunks(int64_t n_est);                                   // workgroups per row of the two row-wise kernels
int metric_input_sdr_blocks(int n_clips);                                // workgroups per clip of the input-SDR kernel, for every entry point
void launch_metric_time_ragged(const float* est, const float* speech, const float* mix, const int64_t* lens, int R, int Tmax,
                               int64_t out_stride, int64_t wave_stride, double* part /* [R][chunks][7] */, hipStream_t s);
void launch_metric_sisdr_ragged(const float* est, const float* speech, const int64_t* lens, int R, int Tmax, int64_t out_stride,
                                int64_t wave_stride, const double* time_part /* launch_metric_time_ragged's */, double* part /* [R][chunks][2] */,
                                hipStream_t s);
void launch_metric_input_sdr_ragged(const float* speech, const float* mix, const MetricClip* clips, int n_clips, int64_t wave_stride,
                                    double* part /* [n_clips][blocks] */, int blocks, hipStream_t s);
void launch_metric_freq_ragged(const FftTables& tb, const float* Yf, const float* Sf, const int64_t* lens, int R, int Tmax,
                               double* part /* [R][blocks][2] */, int blocks, hipStream_t s);
// The time and the spectral sums of segment [ta, te) of a ragged batch cut into segments (bsrnn_evaluate_long_ragged; plan_host.h:
// segment_owned), ADDED into the call's accumulators acc_time [R][METRIC_SEG_SLOTS][7] / acc_freq [R][METRIC_SEG_SLOTS][2], which the caller
// zeroes once: the hops the segment completes and the frames it holds, as far as they are a row's own, of the Ri rows of its alive prefix.
// est points at the segment's first hop of row 0, rows est_stride floats apart; speech, mix are the call's; Yf, Sf the segment-local
// spectra [Ri*(te-ta)][ld].  Segments follow each other on one stream, so a slot's additions have a fixed order.
constexpr int METRIC_SEG_SLOTS = 16;
void launch_metric_ragged_segment(const FftTables& tb, const float* est, int64_t est_stride, const float* speech, const float* mix,
                                  const int64_t* lens, int64_t wave_stride, const float* Yf, const float* Sf, int Ri, int ta, int te,
                                  double* acc_time, double* acc_freq, hipStream_t s);
// Per-hop activity (bsrnn_hop_activity): for hop h < hops[r] of row r, act[r][h] = {mean(est^2 / (mix - est)^2), mean(mix^2)} over its 1024
// samples, (0, 0) from hops[r] to Hmax; hops [R] on the device, null: every row has Hmax hops.  Rows mix_stride / est_stride floats apart.
void launch_hop_activity(const float* mix, int64_t mix_stride, const float* est, int64_t est_stride, const int32_t* hops, int R, int Hmax,
                         double* act /* [R][Hmax][2] */, hipStream_t s);
// The re-mix of an optimizer step (bsrnn_remix_ragged; remix.hip, the definition: remix_host.h): mixture and target of the R rows of the
// table `rows`, each from its run of `terms` (both on the device), columns [0, width) of every row of both outputs in one launch.
void launch_remix_ragged(const RemixRow* rows, const RemixTerm* terms, int R, float* mix, int64_t mix_stride, float* target, int64_t target_stride,
                         int64_t width, hipStream_t s);
// The tri-loss and the SDR of a ragged training step per clip, and their gradients (bsrnn_train_loss_ragged / _backward; the clip table:
// train_ragged_host.h).  y, sfreq, dy [R][2050][Tmax] in the reference layout; xtime, dxtime [R][(Tmax-1)*1024]; speech rows wave_stride
// floats apart; lens [R], clips [n_clips], row_clip [R], gclip [n_clips][2] on the device.  The forward leaves values [n_clips][TV_COUNT] and
// row_sums [R][2] (doubles, on the device) and needs train_loss_partials(R, Tmax) doubles of scratch; the backward writes all of dy and dxtime.
size_t train_loss_partials(int R, int Tmax);
void launch_train_loss_ragged(const float* y, const float* sfreq, const float* xtime, const float* speech, const int64_t* lens,
                              const TrainClip* clips, int n_clips, int R, int Tmax, int64_t wave_stride, double* part, double* values,
                              double* row_sums, hipStream_t s);
void launch_train_loss_ragged_backward(const float* y, const float* sfreq, const float* xtime, const float* speech, const int64_t* lens,
                                       const TrainClip* clips, const int32_t* row_clip, const float* gclip, const double* row_sums, int R,
                                       int Tmax, int64_t wave_stride, float* dy, float* dxtime, hipStream_t s);

// ------------------------------------------------------------------ sample-rate conversion (resample.hip; the definition: resample_host.h)
// One launch serves bsrnn_resample and the streaming resampler.  The input of row r is the concatenation of two segments - a [a0, a1),
// the resampler's carry (rows a_stride apart; absent offline: a0 = a1 = 0), and b [a1, n_total), the caller's block (rows b_stride
// apart; null in a flush) - with zeros in front of 0 and from n_total on.  Outputs j0 .. j0 + n_j - 1 of every row go to out[r][j - j0].
// carry (optional): the launch also writes inputs [c0, n_total) of every row to carry[r][0 ..], the next call's segment a; it must not
// be the buffer a points at.  tab [ld][up] on the device, laid out by output (resample_table_by_output); ld, chunk and tile from resample_tiling().
struct ResampleArgs {
    const float* a; int64_t a_stride, a0;
    const float* b; int64_t b_stride, a1, n_total;
    float* out; int64_t out_stride, j0, n_j;
    const float* tab;
    int up, down, Kh, ld, chunk, tile, n_tiles;
    float* carry; int64_t carry_stride, c0;
};
void launch_resample(ResampleArgs g, int R, hipStream_t s);

// A bank call (bsrnn_resampler_bank_*; the arithmetic: resample_bank_host.h): C rows, each on its own pair, block length and stream
// position, one launch per BANK_GROUP_ROWS rows.  pairs [n_pairs] on the device, written once; carry: two sets of carry_set = C * cap
// floats, rows cap apart, a row reads the set its descriptor names and writes the other; in (null in a flush) / out: rows in_stride /
// out_stride apart, row r reads in[r][0 .. n_in_r) and writes out[r][0 .. n_j_r).  vec is the launcher's.  tiles [n_pairs] on the host:
// the pairs' tile sizes, for the grid.
// THE POINTER FORM (the native session pool's sessions at their own rates): with in_rows / out_rows, tables of C pointers on the
// device, row r reads at in_rows[r] / writes at out_rows[r] instead of in + r * in_stride / out + r * out_stride - a session's own
// buffer.  Either side may have one.  Only the entries of rows that run are read; a row's 16-byte loads then depend on its own pointer.
struct BankPair { const float* tab; int up, down, Kh, ld, chunk, tile; };
struct BankLaunch {
    const BankPair* pairs;
    const float* in; int64_t in_stride;
    float* out; int64_t out_stride;
    float* carry; int64_t cap, carry_set;
    int vec;
    const float* const* in_rows;
    float* const* out_rows;
};
static_assert(sizeof(BankLaunch) <= BANK_ARG_OTHER, "resample_bank_host.h sizes a group of descriptors beside these");
void launch_resample_bank(BankLaunch L, const int* tiles, const BankRow* rows, int C, hipStream_t s);

// ------------------------------------------------------------------ the native session pool's two copies (pool.hip; the plan: pool_host.h)
// tab [n_entries] on the device: one entry per row of every session a round names.  gather: chunk [C][L*1024] row e.row = the FIFO's
// n_fifo samples ++ n_in samples of e.src, zeros to the end of the row (L = 0: the rectangle is not touched), then fifo [C][1024] row
// e.row gets n_pend samples of e.pend_src at pend_off.  scatter: out [C][L*1024] row e.row, samples [out_skip, n_out) -> e.dst.
void launch_pool_gather(const PoolEntry* tab, int n_entries, float* chunk, float* fifo, int L, hipStream_t s);
void launch_pool_scatter(const PoolEntry* tab, int n_entries, const float* out, int L, hipStream_t s);
// The critic's Conv1d(kernel 16, stride 3) layers (bsrnn_critic_conv_*; critic.hip, the definition and the layout: critic_host.h).
// x [C][I][T], w [O][I][16], b [O], y / dy [C][O][T_out]; dx [C][I][T] may be null; scratch: critic_forward_scratch_floats /
// critic_backward_scratch_floats.  y is only read when leaky.
void launch_critic_forward(const float* x, const float* w, const float* b, float* y, float* scratch, int C, int I, int T, int O, int leaky,
                           hipStream_t s);
void launch_critic_backward(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw, float* db, float* scratch,
                            int C, int I, int T, int O, int leaky, hipStream_t s);

// The committed critic (bsrnn_critic_commit / _score; critic_score.hip, the image, the plan and the workspace: critic_score_host.h).
// commit: w [1024][I][16] -> image (csc_image_halves(I) fp16 values) and *wmax = max of the bit patterns of |w| (the caller zeroes it).
// first_h2: layer 1 in fp16x2 from the image, x [C][I][T] in either channel order -> y1 [C][1024][len[0]] (bias and LeakyReLU applied),
// part = the plan's shared block; raises *range_flag when a staged |x| passes 65504.  tail: y4 [C][32][T4] -> score[0].  planar: an
// interleaved x copied into the reference's channel order.
void launch_critic_commit(const float* w, void* image, unsigned* wmax, int I, hipStream_t s);
void launch_critic_first_h2(const float* x, const void* image, const float* bias, float* y1, float* part, int* range_flag, const CscPlan& p,
                            int x_order, hipStream_t s);
void launch_critic_tail(const float* y4, const float* lin_w, const float* lin_b, float* score, int C, int T4, hipStream_t s);
void launch_critic_planar(const float* x, float* out, int C, int I, int T, hipStream_t s);

// The committed critic's gradient (bsrnn_critic_enable_grad / _score_grad / _layer1_dx; critic_grad.hip, the second image, the tiling and
// the workspace: critic_grad_host.h).  dp / dx: the two backward kernels of critic.hip alone - dp = dy * act'(y) over n values, and
// dx [C][I][T] from dp [C][O][T_out] - with no dW beside them.  grad_commit: w [1024][I][16] -> the dx image (cgd_image_halves(I) fp16
// values).  tail_grad: score[0], lin_w, gscale (null: 1) -> gp [32] and dp4 [C][32][T4].  dp_max: as dp (y null: a plain read; dp null:
// nothing written; dy == dp allowed) and *mx = max of the bit patterns of |dp| (the caller zeroes it).  dx_h2: layer 1's dx in fp16x2
// from the image and *mx, written in x_order; raises *range_flag for a non-finite maximum.  scatter: a planar dx into interleaved order.
void launch_critic_dp(const float* dy, const float* y, float* dp, size_t n, hipStream_t s);
void launch_critic_dx(const float* w, const float* dp, float* dx, int C, int I, int T, int O, hipStream_t s);
void launch_critic_grad_commit(const float* w, void* image, int I, hipStream_t s);
void launch_critic_tail_grad(const float* score, const float* lin_w, const float* gscale, float* gp, float* dp4, int C, int T4, hipStream_t s);
void launch_critic_dp_max(const float* dy, const float* y, float* dp, unsigned* mx, size_t n, hipStream_t s);
void launch_critic_dx_h2(const float* dp, const void* image, float* dx, const unsigned* mx, int* range_flag, const CgdPlan& g, int x_order,
                         hipStream_t s);
void launch_critic_scatter(const float* in, float* out, int C, int I, int T, hipStream_t s);

// The committed critic on a padded batch (bsrnn_critic_score_ragged / _score_grad_ragged; the tables, the live tiles and the workspace:
// critic_ragged_host.h): the ragged forms of the launches above.  p / g are the RECTANGLE's plans (R rows of Tmax frames), rows [R] and
// clips [n_clips] the call's device tables.  first_h2_ragged: y1 [R][1024][len[0]], valid below each row's own T1_r.  tail_ragged: one
// score per clip.  tail_grad_ragged: gscale [n_clips] or null -> gp [n_clips][32] and dp4 [R][32][T4max], zeros behind a row's T4_r.
// dp_max_rows: as dp_max, n_row values per row, the maximum into mx[clip of the row] (the caller zeroes the n_clips words).  dx_h2_ragged:
// every s < Tmax of every row is written, zeros behind a row's frames.  planar_ragged: zeros behind a row's frames.
void launch_critic_first_h2_ragged(const float* x, const void* image, const float* bias, float* y1, float* part, int* range_flag, const CscPlan& p,
                                   int x_order, const CrgRow* rows, hipStream_t s);
void launch_critic_tail_ragged(const float* y4, const float* lin_w, const float* lin_b, float* scores, const CrgClip* clips, int n_clips, int T4max,
                               hipStream_t s);
void launch_critic_planar_ragged(const float* x, float* out, int R, int I, int Tmax, const CrgRow* rows, hipStream_t s);
void launch_critic_tail_grad_ragged(const float* scores, const float* lin_w, const float* gscale, float* gp, float* dp4, const CrgClip* clips,
                                    int n_clips, int T4max, hipStream_t s);
void launch_critic_dp_max_rows(const float* dy, const float* y, float* dp, unsigned* mx, const CrgRow* rows, int R, size_t n_row, hipStream_t s);
void launch_critic_dx_h2_ragged(const float* dp, const void* image, float* dx, const unsigned* mx, int* range_flag, const CgdPlan& g, int x_order,
                                const CrgRow* rows, hipStream_t s);

// The critic's input (bsrnn_critic_spectrum; stft4096.hip, the definition and the slab rule: critic_spectrum_host.h): the 4096-point
// analysis of slab q of a call - rows [r0, r1) x frames [t0, t1) of wave (rows `stride` floats apart, n samples each, T frames) - as
// frame-major records scratch [(r - r0) * (t1 - t0) + (t - t0)][4098] (re, im interleaved), then their transpose into
// x [R][4098][T] (real rows, then imaginary rows).
struct CsTables {            // device tables, built in double on the host at the first bsrnn_critic_spectrum of a context
    const float2* tw;        // exp(-2 pi i k / 2048), k < 2048
    const float2* split;     // exp(-2 pi i k / 4096), k <= 2048
    const float* hann;       // periodic Hann(4096)
};
void launch_critic_spectrum_slab(const CsTables& tb, const float* wave, int64_t stride, int64_t n, float scale, float* scratch, float* x, int T,
                                 const CsSlab& q, hipStream_t s);

}  // namespace bsrnn
