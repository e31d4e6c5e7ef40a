// Plain-data descriptors that the host fills at commit time (commit_host.h) and the kernels read (kernels.h includes this file),
// and the constants that the host-side call plan (plan_host.h) shares with the kernels.
// No HIP here: a host compiler takes it as it is.
#pragma once

#if defined(__HIPCC__)
#define BSRNN_HD __host__ __device__
#else
#define BSRNN_HD
#endif

namespace bsrnn {

constexpr int HID = 64;       // band_features (bsrnn.py:60)
constexpr int NFFT = 2048;    // infer.py:31
constexpr int HOPS = 1024;
constexpr int NBINS = 1025;
constexpr int F2 = 2050;      // interleaved re/im columns

// ------------------------------------------------------------------ grouped linear layers
// One job = one nn.Linear of one band.  A launch runs every job of one "layer slot" of the
// per-band MLP chains over all M = C*T frame rows.
struct GemmJob {
    const float* W;      // [N][K] row-major (torch Linear layout), device, K padded to a multiple of 8 floats
    const void* Wp;      // the same matrix as two fp16 pieces, slab-interleaved [N][K32 / 32][2][32] (split_host.h)
    const float* bias;   // [N]
    int N, K;            // K may be 0: y = bias (TrainableConstantModule, bsrnn.py:12-24)
    int x_off;           // column offset of the job's input inside an X row
    int y_off;           // column offset of the output inside a Y row
    int r_off;           // column offset inside the residual row (EPI_RES, EPI_MASK)
    int m_off;           // column offset inside the multiplier / mask-tap row (EPI_MASK)
    int wrow;            // 16-bit elements between consecutive weight rows of Wp
};
// (job index, column-tile index inside the job) of one workgroup of a grouped launch; the kernels read it as an int2
struct GemmTile { int job, tile; };

// How the Linear layers are evaluated (environment BSRNN_GEMM = f32 | fp16x2 | fp16, read once per process).
// fp16 = plain 16-bit operands, one MFMA term, fp32 accumulate (the reduced-precision configuration, not the default).
// The fp32 weights are always resident beside the fp16 pieces: a call whose operands left the fp16x2 range is re-run on
// the exact-fp32 kernels (set_force_f32, per host thread) by the synchronous entry points of api.hip.
// bf16 = plain bf16 operands, one MFMA term, in the fused MLP chains (BASELINE config 2 as it is named; no range limit, 8 significant
// bits); the few launches outside the chains (a band too wide for the LDS image, the block fc of the BSRNN_BAND_FC=gemm flow) then run fp16x2.
enum GemmMode { GEMM_F32 = 0, GEMM_FP16 = 1, GEMM_FP16X2 = 2, GEMM_BF16 = 3 };
// How the recurrent layers evaluate their gate products (environment BSRNN_LSTM = f32 | fp16x2, read once).
enum LstmMode { LSTM_F32 = 0, LSTM_FP16X2 = 2 };
// A call of at most this many frame rows runs its per-band layers on the GEMV kernels (gemv.hip; plan_call, plan_host.h)
constexpr int GEMV_MAX_FRAME_ROWS = 4;

// ------------------------------------------------------------------ fused per-band MLP chains (mlp_chain.hip)
// One workgroup = one band x one block of frame rows, all five Linear layers of BandSplit (bsrnn.py:404-415) or of
// MaskEstimation (bsrnn.py:420-443); intermediates stay in LDS as fp16x2 pieces.
constexpr int CHAIN_LAYERS = 5;
constexpr int CHAIN_CT = 3;                   // feature tiles (32 wide) per wave and layer, at most
constexpr int CHAIN_LDS_EX = 144 * 1024;      // activation images of the workgroup's row tiles
constexpr int CHAIN_LDS_BIAS = 13 * 1024;     // the chain's biases (both together: 157 of the CU's 160 KB)
enum { CHAIN_SPLIT = 0, CHAIN_MASK = 1 };
struct ChainLayer {
    int K16;             // k-steps of 16 (input width rounded up)
    int NTL;             // feature tiles of 32 (output width rounded up); weights and biases beyond N are zero
    int bias_off;        // first bias of the layer inside the chain's bias block (floats)
    int leaky;           // LeakyReLU(0.01) after the layer
    unsigned w_off;      // byte offset of the layer's fragment streams inside ChainDesc::wstream
    int rag;             // 1: the last of the NTL feature tiles (<= 4 real features) is split over the k-steps of all waves (split_host.h)
};
constexpr int CHAIN_RAG_LDS = 8 * 1024;       // LDS behind the activation images that the partial sums of such a tile need
struct ChainDesc {
    ChainLayer L[CHAIN_LAYERS];
    const void* wstream; // per layer, per wave wn: for tile t = wn + NW c, for ks, for piece: 64 lanes x 8 fp16 (split_host.h)
    const float* bias;   // the five bias vectors, each padded with zeros to NTL * 32 (constant band: the constant itself)
    int nbias;
    int NW, RT;          // groups of NW waves share the feature tiles of their RT row tiles (of 32 rows): mlp_chain.hip.
                         // RT = 3: the 48-row geometry on 16 x 16 x 32 MFMAs (K16 then counts k-steps of 32, NTL tiles of 16)
    int plane_units;     // 512-byte units of one piece of one row tile's activation image: max(2 K16, 4 NTL) over the layers
    int in_off;          // first column of the band inside an input row (SPLIT: spectrum row, MASK: b * 64 of a Z row)
    int K0;              // valid input columns, a multiple of 8 (beyond: zeros)
    int p_off;           // first column of the band in the band-padded rows (P, spectrum, output)
    int a8;              // band width in columns rounded up to 8: what is written to P / Y (pad columns exactly zero)
    int z_off;           // first column of the band inside a Z row
    int constant;        // zero-width band (TrainableConstantModule, bsrnn.py:12-24): Z[:, z_off .. +64) = bias[0 .. 64)
    int zpad;            // 16 x 16 geometry: the image's k-units that no layer output covers but the next layer's K loop reads are
                         // zeroed first (chain_body48 ZPAD): set when a layer feeding another has N % 32 != 0 (its output ends
                         // after an odd number of feature tiles of 16, the next K loop runs whole k-steps of 32); always on the
                         // 64-row body
};
// rows per workgroup of a descriptor (32 RT GR; 256 for a constant band)
BSRNN_HD inline int chain_rows(const ChainDesc& d) { return d.constant ? 256 : (d.RT >= 3 ? 16 * d.RT : 32 * d.RT * (8 / d.NW)); }   // RT >= 3: row tiles of 16 (16 x 16 x 32 geometry: 48 or 80 rows)

// Overlapped dual path (kernels.h): a progress word is epoch << OVL_EPOCH_SHIFT | groups of four steps done
constexpr int OVL_EPOCH_SHIFT = 12;            // groups of four steps per launch < 4096 (frames < 16 384: plan_call checks, plan_host.h)

// positions (bands) the LDS images of the band-block kernel for a few sequences hold (launch_band_block_small, kernels.h); longer
// band tables take the general kernels
constexpr int BS_MAXL = 16;

}  // namespace bsrnn
