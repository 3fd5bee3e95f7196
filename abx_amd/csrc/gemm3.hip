// fp32 GEMM on the float16 matrix cores by operand splitting ("split-f16"): the large contractions of the pair stack.
//
// An fp32 product is evaluated from three exact partial products on v_mfma_f32_32x32x16_f16 with fp32 accumulation
//     x y ~ a1 p2 + a0 p1 + a0 p0                              (smallest terms first)
//     A side (two pieces):   x' = x 2^-4,  a0 = f16(x'),  a1 = f16((x' - a0) 2^11)
//     B side (two planes):   y' = y 2^e,   p0 = f16(y'),  p1 = f16(y' - p0);  p2 = f16(p0 2^-11) is derived in registers
// Each f16 x f16 product is exact in fp32.  A piece pair holds 23 significant bits and the dropped term a1 p1 2^-11 is <= 2^-22 |x y|,
// mean zero: measured against fp64 (tests/test_gpu_kernels.py) the error is that of the exact v_mfma_f32_32x32x2_f32 kernel of
// gemm.hip, while the matrix cores run 16/3 = 5.3x faster than their fp32 rate.  The power-of-two scales keep the pieces normal
// float16 numbers (range contract and what happens beyond it: include/abx_hip.h, "Split-f16 operands").  The
// exact kernel remains selectable (AbxGemm.exact).  Rounds 1-2 used three bf16 pieces per operand and six products.
//
// Data movement is all asynchronous global->LDS DMA (global_load_lds_dwordx4): no operand passes through VGPRs on its way
// to LDS (no staging registers, no ds_write pass, no vector address arithmetic); the k-loop waits with an explicit
// s_waitcnt + raw s_barrier and is double buffered.
//   A  fp32, k-contiguous rows (AMODE 0): 2 stages [BM][16] fp32 (64-byte rows, 16-byte slots XOR-swizzled through
//      the SOURCE address).  Every wave reads its own rows as fp32 fragments and splits them in registers right in front of
//      the MFMAs; the LayerNorm statistics (inline mode), the mean shift and relu-on-load are applied to those registers.
//      Optional pair transposition of the rows (a_pair_transpose): the DMA source address is per lane, so the incoming
//      TriangleMultiplication reads z[k][i] rows in (i,k) order for free.
//   A  fp32, row-contiguous / channel-major (AMODE 1): 2 stages [16 k][BM] fp32, fragments by 4-byte LDS reads.
//   A  pre-split pieces (AMODE 2: planes 0, 1) and B always pre-split planes, k-TILED in memory: [K/16][2][rows][16] so that the
//      32 bytes a row contributes to a k-tile sit next to the neighbouring rows' (full 128-byte lines per DMA instead of a
//      quarter line per row, which the 32 KB L1 cannot keep until the next k-tile): weights from abx_split_weights_f16, or
//      activations written by a producer GEMM with C_split (the TriangleMultiplication einsum seqformer.py:490-493 takes
//      both operands this way).  LDS image [plane][row][32 B], the two 16-byte halves swapped on odd row-octets:
//      conflict-free ds_read_b128 fragment reads (lane -> row, lane >> 5 -> k half).
// Requirements (abx_gemm falls back to the exact kernel otherwise): K % 16 == 0, 16-byte aligned operand rows.
// Epilogue: gemm_epilogue.h (shared with gemm.hip).  Main loop: gemm3_mainloop.h (shared with tails.hip).
#include "common.h"
#include "abx_hip.h"
#include "gemm_epilogue.h"
#include "gemm3_mainloop.h"
#include "grid_map.h"

namespace {

template <int BM, int BN, int WM, int WN, int AMODE, bool EDGE, bool TS, bool OLN = false, bool PROBE = true, int RING = 2>
__device__ __forceinline__ void gemm3_block(const AbxGemm& g, float* smem, int mt, int nt, int b) {
    constexpr int TM = WM / 32, TN = WN / 32;
    f32x16 acc[TM][TN];
    float ls[TM], lq[TM], lsh[TM];
    gemm3_mainloop<BM, BN, WM, WN, AMODE, false, true, RING>(g, smem, mt, nt, b, acc, ls, lq, lsh);
    float* st_lds = smem;                                   // [BM][2]
    const bool stats = gemm3_row_stats<BM, BN, WM, WN, EDGE>(g, st_lds, mt, b, ls, lq);
    __syncthreads();
    gemm_epilogue<BM, BN, WM, WN, EDGE, TS, OLN, PROBE>(g, st_lds, smem + 2 * BM, acc, mt * BM, nt * BN, b, stats);
}

// Dual GEMM (the TriangleMultiplication tail, seqformer.py:496-503): out = epi(A' B) * sigmoid(LN(A2) B2 + bias2) (+ resid).
// Two main loops over the same output tile into two accumulator sets: the channel-major product (AMODE 1) against proj_out, then
// the rows of z (k-contiguous, inline LayerNorm) against the final-gate weights; the gate never travels through HBM and z is
// read once for both the gate and the residual.
template <int BM, int BN, int WM, int WN, bool EDGE>
__device__ __forceinline__ void gemm3_dual_block(const AbxGemm& g, float* smem, int mt, int nt, int b) {
    constexpr int TM = WM / 32, TN = WN / 32;
    f32x16 acc[TM][TN], acc2[TM][TN];
    float ls[TM], lq[TM], ls2[TM], lq2[TM], lsh[TM], lsh2[TM];
    AbxGemm g2 = g;                                          // operand view of the gate GEMM
    g2.A = g.A2; g2.sAb = g.sA2b; g2.sAm = g.sA2m; g2.sAk = 1; g2.K = g.K2;
    g2.A_split = nullptr; g2.a_relu = 0; g2.a_pair_transpose = 0; g2.a_pair = g.pair_Lp > 0 ? 1 : 0;
    g2.B_split = g.B2_split; g2.sB3p = g.sB23p; g2.sB3n = g.sB23n; g2.sB3k = g.sB23k; g2.sB3b = 0;
    g2.ln_csum = g.ln2_csum; g2.ln_stats = nullptr; g2.batch_inner = 0; g2.b_exp = g.b2_exp;
    if (g.sAk == 1) gemm3_mainloop<BM, BN, WM, WN, 0>(g, smem, mt, nt, b, acc, ls, lq, lsh);
    else gemm3_mainloop<BM, BN, WM, WN, 1>(g, smem, mt, nt, b, acc, ls, lq, lsh);
    gemm3_mainloop<BM, BN, WM, WN, 0>(g2, smem, mt, nt, b, acc2, ls2, lq2, lsh2);
    float* st_lds = smem;                                   // [BM][2] + [BM][2]
    const bool stats = gemm3_row_stats<BM, BN, WM, WN, EDGE>(g, st_lds, mt, b, ls, lq);
    gemm3_row_stats<BM, BN, WM, WN, EDGE>(g2, st_lds + 2 * BM, mt, b, ls2, lq2);
    __syncthreads();
    gemm_epilogue<BM, BN, WM, WN, EDGE, false>(g, st_lds, smem + 4 * BM, acc, mt * BM, nt * BN, b, stats, &acc2, st_lds + 2 * BM);
}

// Round 6: the same dual GEMM with ONE walk over the rows of z.  The 128 x 96 tiles above give every row tile two blocks (one per column
// half) that each walk the product rows AND the z rows: the A side of both main loops (DMA from the fabric, fragment reads, LayerNorm
// partial sums, f16 splits) is paid twice per row, 9 MFMAs per k-step.  Under the board's power limit that is what the launch costs
// (profiles/r06a_power_limit.txt; the gated attention tail gained 11 % from the same change).  Here a block owns 128 rows and all
// 192 columns:
//   gate walk   LN(z) against the final-gate weights for all 192 columns (128 x 192 tile, 18 MFMAs per k-step), 96 accumulator
//               registers, turned into the gate VALUES sigmoid(.) in place and kept;
//   two passes  over the output columns (0 .. 95, 96 .. 191): the product rows against proj_out into 48 accumulator registers, then the
//               epilogue of that half: folded LayerNorm, bias, x the kept gate values, + z, store.
// z is walked once instead of twice, the product rows twice as before.  Every accumulator receives the products of the two-tile form
// in the same order and the gate is the same expression: bit-identical results.  MEASURED SLOWER (10.97 vs 10.30 ms at 100 samples of
// L = 352, profiles/r06c_kb_dual.txt): 96 + 48 live accumulator registers leave two blocks per CU where the two-tile form runs three;
// kept behind ABX_TUNE_DUAL_1WALK as the record of the experiment and a cross-check (test_gemm_dual_walk_variants_bit_identical).
template <bool EDGE>
__device__ __forceinline__ void gemm3_dual1_block(const AbxGemm& g, float* smem, int mt, int b) {
    constexpr int BM = 128, BN = 192, WM = 32, BH = 96, TH = BH / 32, TN = BN / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    AbxGemm g2 = g;                                          // operand view of the gate GEMM
    g2.A = g.A2; g2.sAb = g.sA2b; g2.sAm = g.sA2m; g2.sAk = 1; g2.K = g.K2;
    g2.A_split = nullptr; g2.a_relu = 0; g2.a_pair_transpose = 0; g2.a_pair = g.pair_Lp > 0 ? 1 : 0;
    g2.B_split = g.B2_split; g2.sB3p = g.sB23p; g2.sB3n = g.sB23n; g2.sB3k = g.sB23k; g2.sB3b = 0;
    g2.ln_csum = g.ln2_csum; g2.ln_stats = nullptr; g2.batch_inner = 0; g2.b_exp = g.b2_exp;
    float* st_lds = smem;                                   // [BM][2] (product rows) + [BM][2] (z rows)
    f32x16 gatev[1][TN];
    {
        float ls2[1], lq2[1], lsh2[1];
        gemm3_mainloop<BM, BN, WM, BN, 0, false, true, 2>(g2, smem, mt, 0, b, gatev, ls2, lq2, lsh2);
        gemm3_row_stats<BM, BN, WM, BN, EDGE>(g2, st_lds + 2 * BM, mt, b, ls2, lq2);
        __syncthreads();
        const float* st2 = st_lds + 2 * BM;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = j * 32 + (lane & 31);
            const bool nok = !EDGE || n < g.N;
            const float csum2 = nok ? g.ln2_csum[n] : 0.f, bias2 = (g.bias2 && nok) ? g.bias2[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = wave * WM + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                // (gemm_epilogue.h, the acc2 path: the same expression, the same rounding)
                const float gv = st2[2 * ml + 1] * (gatev[0][j][r] - st2[2 * ml] * csum2) + bias2;
                gatev[0][j][r] = sigmoidf_(gv);
            }
        }
        __syncthreads();                                    // (the statistics are read: the next main loop's stages overlay them)
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        f32x16 acc[1][TH];
        float ls[1], lq[1], lsh[1];
        if (g.sAk == 1) gemm3_mainloop<BM, BH, WM, BH, 0, false, true, 2>(g, smem, mt, half, b, acc, ls, lq, lsh);
        else gemm3_mainloop<BM, BH, WM, BH, 1, false, true, 2>(g, smem, mt, half, b, acc, ls, lq, lsh);
        const bool stats = gemm3_row_stats<BM, BH, WM, BH, EDGE>(g, st_lds, mt, b, ls, lq);
        __syncthreads();
        gemm_epilogue<BM, BH, WM, BH, EDGE, false, false, true>(g, st_lds, smem + 4 * BM, acc, mt * BM, half * BH, b, stats, nullptr, nullptr,
                                                                reinterpret_cast<const f32x16 (*)[1][TH]>(&gatev[0][half * TH]));
        if (half == 0) __syncthreads();                     // (the scratch and the statistics are read: the next main loop overlays them)
    }
}

__global__ __launch_bounds__(256, 2) void gemm3_dual1_kernel(const AbxGemm g) {
    constexpr int OPER = (2 * 128 * 64 + 2 * 2 * 192 * 32) / 4;
    constexpr int EPI = 4 * 128 + 4 * 32 * (3 * 32 + 4);
    __shared__ __attribute__((aligned(16))) float smem[OPER > EPI ? OPER : EPI];
    const int ntm = (g.M + 127) / 128;
    const unsigned wgid = xcd_contiguous(blockIdx.x, gridDim.x);
    const int b = (int)(wgid / (unsigned)ntm), mt = (int)(wgid - (unsigned)b * (unsigned)ntm);
    const ClockProbe probe(g.clock_probe);
    if ((mt + 1) * 128 <= g.M && g.N == 192) gemm3_dual1_block<false>(g, smem, mt, b);
    else gemm3_dual1_block<true>(g, smem, mt, b);
    probe.finish();
}

template <int BM, int BN, int WM, int WN, int AMODE, bool TS, int MINW>
__global__ __launch_bounds__(256, MINW) void gemm3_kernel(const AbxGemm g) {
    constexpr int A_IMG = AMODE == 2 ? 2 * BM * 32 : BM * 64;
    constexpr int A_STAGE = A_IMG;
    constexpr int B_STAGE = 2 * BN * 32;
    constexpr int RING = 2;       // (3 stages at 3 blocks per CU, 4 at 2: 4.08 / 4.67 ms against 3.68 at N = 768, K = 192, 20 samples - DESIGN.md 4c)
    constexpr int OPER = RING * (A_STAGE + B_STAGE) / 4;                           // floats
    constexpr int TNW = WN / 32, TGW = TNW > 3 ? (TNW % 3 == 0 ? 3 : 2) : TNW;      // epilogue column group (gemm_epilogue.h)
    constexpr int SCR = 4 * 32 * ((TS ? WM : TGW * 32) + 4);
    constexpr int EPI = 2 * BM + SCR;
    __shared__ __attribute__((aligned(16))) float smem[OPER > EPI ? OPER : EPI];
    // 1-D grid over (batch, m-tile, n-tile).  XCD-aware remap (blocks are placed round-robin over the 8 XCDs): every XCD gets a
    // contiguous range of tiles, so the N-tiles that share an A panel - and all tiles of one batch entry of the
    // triangle-multiplication contraction - meet in one private L2.  Bijective for any grid size.
    const int ntn = (g.N + BN - 1) / BN, ntm = (g.M + BM - 1) / BM;
    const int per_batch = ntn * ntm;
    const ClockProbe probe(g.clock_probe);
    constexpr bool PROBE = !(BM == 128 && BN == 128 && MINW >= 4);      // (no register for it at four blocks per CU: gemm_epilogue.h)
    // (32-bit: the dispatch keeps the grid below 2^31 tiles; a 64-bit division is ~80 instructions in front of the block's first DMA)
    const unsigned wgid = (g.tune & ABX_TUNE_NO_REMAP) ? blockIdx.x : xcd_contiguous(blockIdx.x, gridDim.x);
    const int b = (int)(wgid / (unsigned)per_batch);
    const int rem = (int)(wgid - (unsigned)b * (unsigned)per_batch);
    const int mt = rem / ntn, nt = rem % ntn;
    const bool interior = (mt + 1) * BM <= g.M && (nt + 1) * BN <= g.N;
    if (interior) gemm3_block<BM, BN, WM, WN, AMODE, false, TS, false, PROBE, RING>(g, smem, mt, nt, b);
    else gemm3_block<BM, BN, WM, WN, AMODE, true, TS, false, PROBE, RING>(g, smem, mt, nt, b);
    probe.finish();
}

// A 128 x 128 plain-store GEMM with a SIDE GEMM in its grid: the skinny (N <= 32, transposed store) projection of the SAME rows - the
// triangle attention's pair bias next to its q | k | v | gate projection (seqformer.py:520-531).  Side tiles (128 rows x 32 columns,
// the block body of the narrow kernel) are dealt evenly between the main tiles in launch order, so a side tile runs while the main
// tiles of the same rows are resident on its XCD and takes its A panel from that L2 instead of a second 9.5 GB HBM read of z in a
// launch of its own.  Every tile's arithmetic is what the two separate launches do: results are bit-identical.
__global__ __launch_bounds__(256, 4) void gemm3_side_kernel(const AbxGemm g, const AbxGemm s2) {
    constexpr int BM = 128, BN = 128;
    __shared__ __attribute__((aligned(16))) float smem[35840 / 4];
    const unsigned ntn = (g.N + BN - 1) / BN, ntm = (g.M + BM - 1) / BM, per_batch = ntn * ntm;
    const unsigned stm = (s2.M + BM - 1) / BM, ts = stm * (unsigned)s2.batch;
    const unsigned total = gridDim.x, wgid = xcd_contiguous(blockIdx.x, total);
    // slot w is a side tile when floor((w + 1) ts / total) > floor(w ts / total); it is side tile floor(w ts / total)
    const unsigned sw = (unsigned)(((unsigned long long)wgid * ts) / total), sw1 = (unsigned)(((unsigned long long)(wgid + 1) * ts) / total);
    if (sw1 > sw) {
        const int b = (int)(sw / stm), mt = (int)(sw - (unsigned)b * stm);
        if ((mt + 1) * BM <= s2.M && 32 <= s2.N) gemm3_block<BM, 32, 32, 32, 0, false, true>(s2, smem, mt, 0, b);
        else gemm3_block<BM, 32, 32, 32, 0, true, true>(s2, smem, mt, 0, b);
        return;
    }
    const unsigned w = wgid - sw;
    const int b = (int)(w / per_batch);
    const int rem = (int)(w - (unsigned)b * per_batch);
    const int mt = rem / (int)ntn, nt = rem % (int)ntn;
    if ((mt + 1) * BM <= g.M && (nt + 1) * BN <= g.N) gemm3_block<BM, BN, 32, 128, 0, false, false, false, false>(g, smem, mt, nt, b);
    else gemm3_block<BM, BN, 32, 128, 0, true, false, false, false>(g, smem, mt, nt, b);
}

// Probe (round 6, ABX_TUNE_NARROW_RING_MASK): the skinny N <= 32 projections - HBM streams of 9.5 / 6.3 GB at 4.2 - 4.5 TB/s - with a deeper operand ring
// (RING k-tiles of A in flight per block instead of one); bit-identical to gemm3_kernel<128, 32, 32, 32, 0, TS, 6>
template <bool TS, int RING, int MINW>
__global__ __launch_bounds__(256, MINW) void gemm3_narrow_ring_kernel(const AbxGemm g) {
    constexpr int BM = 128, BN = 32;
    constexpr int OPER = RING * (BM * 64 + 4096) / 4;
    constexpr int EPI = 2 * BM + 4 * 32 * ((TS ? 32 : 32) + 4);
    __shared__ __attribute__((aligned(16))) float smem[OPER > EPI ? OPER : EPI];
    const int ntm = (g.M + BM - 1) / BM;
    const unsigned wgid = xcd_contiguous(blockIdx.x, gridDim.x);
    const int b = (int)(wgid / (unsigned)ntm), mt = (int)(wgid - (unsigned)b * (unsigned)ntm);
    if ((mt + 1) * BM <= g.M && BN <= g.N) gemm3_block<BM, BN, 32, 32, 0, false, TS, false, true, RING>(g, smem, mt, 0, b);
    else gemm3_block<BM, BN, 32, 32, 0, true, TS, false, true, RING>(g, smem, mt, 0, b);
}

// Linear -> LayerNorm over the output row (out_ln): k-contiguous fp32 A, one n-tile, plain store
template <int BM, int BN, int WM, int WN, int MINW>
__global__ __launch_bounds__(256, MINW) void gemm3_oln_kernel(const AbxGemm g) {
    constexpr int OPER = (2 * BM * 64 + 2 * 2 * BN * 32) / 4;
    constexpr int TNW = WN / 32, TGW = TNW > 3 ? (TNW % 3 == 0 ? 3 : 2) : TNW;
    constexpr int EPI = 2 * BM + 4 * 32 * (TGW * 32 + 4);
    __shared__ __attribute__((aligned(16))) float smem[OPER > EPI ? OPER : EPI];
    const int ntm = (g.M + BM - 1) / BM;
    const unsigned wgid = xcd_contiguous(blockIdx.x, gridDim.x);
    const int b = (int)(wgid / (unsigned)ntm), mt = (int)(wgid - (unsigned)b * (unsigned)ntm);
    const bool interior = (mt + 1) * BM <= g.M && BN <= g.N;
    if (interior) gemm3_block<BM, BN, WM, WN, 0, false, false, true>(g, smem, mt, 0, b);
    else gemm3_block<BM, BN, WM, WN, 0, true, false, true>(g, smem, mt, 0, b);
}

template <int BM, int BN, int WM, int WN, int MINW>
__global__ __launch_bounds__(256, MINW) void gemm3_dual_kernel(const AbxGemm g) {
    constexpr int A_STAGE = BM * 64, B_STAGE = 2 * BN * 32;
    constexpr int OPER = (2 * A_STAGE + 2 * B_STAGE) / 4;
    constexpr int TNW = WN / 32, TGW = TNW > 3 ? (TNW % 3 == 0 ? 3 : 2) : TNW;
    constexpr int EPI = 4 * BM + 4 * 32 * (TGW * 32 + 4);
    __shared__ __attribute__((aligned(16))) float smem[OPER > EPI ? OPER : EPI];
    const int ntn = (g.N + BN - 1) / BN, ntm = (g.M + BM - 1) / BM;
    const unsigned wgid = xcd_contiguous(blockIdx.x, gridDim.x);
    const int per_batch = ntn * ntm;
    const int b = (int)(wgid / (unsigned)per_batch);
    const int rem = (int)(wgid - (unsigned)b * (unsigned)per_batch);
    const int mt = rem / ntn, nt = rem % ntn;
    const bool interior = (mt + 1) * BM <= g.M && (nt + 1) * BN <= g.N;
    if (interior) gemm3_dual_block<BM, BN, WM, WN, false>(g, smem, mt, nt, b);
    else gemm3_dual_block<BM, BN, WM, WN, true>(g, smem, mt, nt, b);
}

// Fused two-layer transition (seqformer.py:358-376: LayerNorm -> Linear(4x) -> ReLU -> Linear, + residual) for 128 rows per block:
//     out = relu(LN(A) W1 + b1) W2 + b2 (+ resid)          A: k-contiguous fp32 rows (K = g.K), hidden width g.N, output width g.N2
// The hidden activations never exist in memory.  The hidden dimension is walked in chunks of 128:
//   GEMM 1 of a chunk is the ordinary main loop with the MFMA operands SWAPPED, so a wave's accumulators hold the TRANSPOSED tiles
//   H^T[hidden][row]: lane = row, registers = 16 hidden channels.  Folded LayerNorm (the row statistics are lane-local in this
//   orientation), bias and ReLU are applied to the registers, which are then split into f16 pieces and ARE the A operand of GEMM 2
//   (lane = row, 8 k values per k-step): a 32 x 32 tile feeds two k-steps whose k slots (lane half h, slot i) hold the hidden
//   channel 8 (i >> 2) + 4 h + (i & 3) of a 16-channel k-tile.  The W2 planes are stored with exactly that order inside every
//   k-tile (AbxGemm.B2_split of an mlp descriptor; abx_amd.ops.permute_k16), so its fragments are the usual 16-byte reads.
//   GEMM 2 streams the chunk's 8 k-tiles of W2 (all N2 <= 192 columns) through a double-buffered LDS stage of its own; its first
//   tile is requested before GEMM 1 of the chunk starts.
// A is read from HBM once (the 6 chunk walks of a block hit the L2 / MALL), the hidden never leaves the CU, the output rows are
// written once: 2 x 192 floats of HBM traffic per pair row instead of 2 x 192 + 2 x 768.
constexpr int MLP_NH = 768;                                                  // widest hidden layer of the fused transition (LDS table)
template <bool EDGE>
__device__ __forceinline__ void gemm3_mlp_block(const AbxGemm& g, float* smem, int mt, int b) {
    constexpr int BM = 128, BN = 128, WM = 32, WN = 128, BN2 = 192, TN2 = BN2 / 32;
    constexpr int G1_BYTES = 2 * (BM * 64 + 2 * BN * 32);                    // stages of GEMM 1 (A fp32 + W1 planes)
    constexpr int B2_IMG = 2 * BN2 * 32;                                     // one k-tile of W2: [2][192][16] f16
    constexpr int NL2 = (B2_IMG + 4095) / 4096;
    char* W2s = reinterpret_cast<char*>(smem) + G1_BYTES;                    // 2 stages
    // column sums and biases of the first layer in LDS [2][768] (read per k-step of GEMM 2: as global loads every step waited out an L2
    // round trip - and, in issue order, the weight DMA requested before them)
    float* cst = reinterpret_cast<float*>(W2s + 2 * B2_IMG);
    for (int i = threadIdx.x; i < MLP_NH; i += 256) {
        cst[i] = i < g.N ? g.ln_csum[i] : 0.f;
        cst[MLP_NH + i] = (i < g.N && g.bias) ? g.bias[i] : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    f32x16 acc2[1][TN2];
#pragma unroll
    for (int t = 0; t < TN2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[0][t][r] = 0.f;
    // DMA sources of the W2 k-tiles (all N2 columns)
    unsigned offs2[NL2];
    plane_sources<BN2, NL2>(g.sB23p, g.sB23n, 0, g.N2, offs2);
    const char* base2 = reinterpret_cast<const char*>(g.B2_split);
    const long long step2 = g.sB23k * 2;
    auto issue_w2 = [&](int ktile, int stage) {
        char* dst = W2s + stage * B2_IMG + wave * NL2 * 1024;
        const char* src = base2 + ktile * step2;
#pragma unroll
        for (int i = 0; i < NL2; ++i)
            if (B2_IMG % 4096 == 0 || (wave * NL2 + i) * 1024 < B2_IMG) glds16(src + offs2[i], dst + i * 1024);
    };
    // fragment of n-tile t: + t * 1024 bytes (32 rows of 32 bytes; the half swap of plane_off depends on (row >> 3) & 1 only)
    const int offB2 = plane_off<BN2>(0, lane & 31, h);
    constexpr int TG2 = 2;                                                   // n-tiles per fragment group (register budget)
    const bool rows_live = mt * BM + wave * WM < g.M;

    float ls[1], lq[1], lsh[1] = {0.f};
    float rstd = 0.f, dmean = 0.f;
    const int nchunk = (g.N + BN - 1) / BN;
    for (int c = 0; c < nchunk; ++c) {
        issue_w2(c * (BN / 16), 0);                                          // first W2 k-tile of the chunk: lands under GEMM 1
        f32x16 acc1[1][BN / 32];
        if (c == 0) {
            gemm3_mainloop<BM, BN, WM, WN, 0, true, true>(g, smem, mt, c, b, acc1, ls, lq, lsh);
            // row statistics of this lane's row (the two lane halves hold the two k halves)
            const float invK = 1.0f / (float)g.K;
            const float sm = ls[0] + __shfl_xor(ls[0], 32, 64), sq = lq[0] + __shfl_xor(lq[0], 32, 64);
            dmean = sm * invK;
            rstd = 1.0f / sqrtf(fmaxf(sq * invK - dmean * dmean, 0.f) + g.ln_eps);
        } else {
            gemm3_mainloop<BM, BN, WM, WN, 0, true, false>(g, smem, mt, c, b, acc1, ls, lq, lsh);
        }
        // (the main loop ended with every DMA drained - the W2 tile included - and a block barrier)
        const int hid0 = c * BN;
#pragma unroll
        for (int j = 0; j < BN / 32; ++j) {
            // ---- H^T tile j: folded LayerNorm, bias, ReLU, split -> A fragments of two k-steps (one k-step = 8 registers of the tile),
            // each followed by its k-tile of GEMM 2
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                u32x4 hf[2];
                {
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int hc = hid0 + j * 32 + 8 * (2 * s2 + q) + 4 * h;    // 4 consecutive hidden channels
                        const int hcl = min(hc, MLP_NH - 4);                 // (channels beyond N: zeros in the table, masked below)
                        const f32x4 cs = *reinterpret_cast<const f32x4*>(cst + hcl), bi = *reinterpret_cast<const f32x4*>(cst + MLP_NH + hcl);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float x = rstd * (acc1[0][j][8 * s2 + 4 * q + e] - dmean * cs[e]) + bi[e];
                            x = relu_keep_nan(x);
                            v[4 * q + e] = (hc + e < g.N) ? x : 0.f;
                        }
                    }
                    // the hidden activations enter GEMM 2 as UNLIFTED pieces of h 2^4 (a0 = f16(h'), a1 = f16(h' - a0): what split2b writes
                    // for plane operands), so its three terms a1 p0 + a0 p1 + a0 p0 need no p2 = p0 2^-11 derived from the W2 fragments
                    // (192 v_pk_mul_f16 per chunk walk and 8 registers less).  |h| < 4094 (beyond: NaN -> the range probe -> the exact
                    // kernels); 22 significant bits from |h| = 2^-7, 2^-29 absolute below - post-ReLU hidden values next to an O(1) sum
                    unsigned q0[4], q1[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) split2b(v[2 * e], v[2 * e + 1], q0[e], q1[e]);
                    hf[0] = u32x4{q0[0], q0[1], q0[2], q0[3]};
                    hf[1] = u32x4{q1[0], q1[1], q1[2], q1[3]};
                }
                const int kl = 2 * j + s2;                                   // k-tile of the chunk, stage kl & 1
                const int knext = c * (BN / 16) + kl + 1;
                if (kl + 1 < BN / 16 && knext * 16 < g.N) issue_w2(knext, (kl + 1) & 1);
                const char* ws = W2s + (kl & 1) * B2_IMG + offB2;
                if (rows_live && (c * (BN / 16) + kl) * 16 < g.N) {
#pragma unroll
                    for (int t0 = 0; t0 < TN2; t0 += TG2) {
                        u32x4 wb[TG2][2];
#pragma unroll
                        for (int t = 0; t < TG2; ++t)
#pragma unroll
                            for (int p = 0; p < 2; ++p) wb[t][p] = *reinterpret_cast<const u32x4*>(ws + (t0 + t) * 1024 + p * (BN2 * 32));
                        // smallest first: a1 p0, a0 p1, a0 p0
                        constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};
#pragma unroll
                        for (int term = 0; term < 3; ++term)
#pragma unroll
                            for (int t = 0; t < TG2; ++t)
                                acc2[0][t0 + t] = mfma_split(hf[TA[term]], wb[t][TB[term]], acc2[0][t0 + t]);
                    }
                }
                wait_vm_and_barrier<0>();
            }
        }
    }
    {
        const float cs2 = __builtin_ldexpf(1.0f, -4 - g.b2_exp);             // (the hidden went in as h 2^4: split2b)
#pragma unroll
        for (int t = 0; t < TN2; ++t) acc2[0][t] *= cs2;
    }
    // ---- epilogue: + bias2 (+ resid), plain store.  A view of the descriptor whose "GEMM" is the second layer.
    AbxGemm g2 = g;
    g2.N = g.N2; g2.bias = g.bias2; g2.ln_csum = nullptr; g2.ln_stats = nullptr; g2.act = 0; g2.alpha = 1.0f;
    __syncthreads();
    gemm_epilogue<BM, BN2, WM, BN2, EDGE, false>(g2, smem, smem + 2 * BM, acc2, mt * BM, 0, b, false);
}

template <int MINB>
__global__ __launch_bounds__(256, MINB) void gemm3_mlp_kernel(const AbxGemm g) {
    constexpr int OPER = (2 * 128 * 64 + 2 * 2 * 128 * 32 + 2 * 2 * 192 * 32) / 4 + 2 * MLP_NH;           // floats (stages + the constants table)
    constexpr int EPI = 2 * 128 + 4 * 32 * (3 * 32 + 4);
    __shared__ __attribute__((aligned(16))) float smem[OPER > EPI ? OPER : EPI];
    const int ntm = (g.M + 127) / 128;
    const unsigned wgid = xcd_contiguous(blockIdx.x, gridDim.x);
    const int b = (int)(wgid / (unsigned)ntm), mt = (int)(wgid - (unsigned)b * (unsigned)ntm);
    const ClockProbe probe(g.clock_probe);
    if ((mt + 1) * 128 <= g.M && g.N2 == 192) gemm3_mlp_block<false>(g, smem, mt, b);
    else gemm3_mlp_block<true>(g, smem, mt, b);
    probe.finish();
}

// Gated tail of the TriangleAttention (seqformer.py:300-312: gate = sigmoid(gate_proj(LN z)), out = proj_out(gate * o), z += out) for 128
// rows per block, in the shape of the fused transition above:
//     out = (sigmoid(LN(A) Wg + bg) * G) Wo + bo (+ resid)        A: k-contiguous fp32 rows (the pair rows z, K = g.K), G = g.gate: the
//                                                                attention output o, [M][N] fp32 rows; N = g.N gate channels, N2 outputs
// The gate never exists in memory (9.5 GB written by the q | k | v | gate projection and read back by the attention kernel per block at
// 100 samples of L = 352) and the output projection is no launch of its own.  The gate channels are walked in chunks of 96:
//   GEMM 1 of a chunk = the main loop with swapped MFMA operands: the accumulators hold the transposed tiles gate^T[channel][row], lane =
//   row; folded LayerNorm (lane-local statistics), bias, sigmoid on the registers;
//   the G operand streams as k-tiles [128 rows][16 channels] fp32 through a double-buffered LDS stage of its own (DMA, the A-stage layout of
//   the main loop); a lane reads the 8 channels its 8 gate registers of a k-step stand for (channels 8 q + 4 h + e of the 16-tile: the
//   k order of permute_k16), multiplies, splits (unlifted pieces of v 2^4: split2b) - that IS the A operand of GEMM 2;
//   GEMM 2 streams the W_o planes (k order permuted inside every 16-tile like the fused transition's second layer).
constexpr int GT_NG = 192;                                                   // gate channels (LDS table)
template <bool EDGE>
__device__ __forceinline__ void gemm3_gtail2w_block(const AbxGemm& g, float* smem, int mt, int b) {
    constexpr int BM = 128, BN = 96, WM = 32, WN = 96, BN2 = 192, TN2 = BN2 / 32;
    constexpr int G1_BYTES = 2 * BM * 64 + 2 * 2 * BN * 32;                  // stages of GEMM 1 (A fp32 + gate-weight planes)
    constexpr int B2_IMG = 2 * BN2 * 32;                                     // one k-tile of W_o: [2][192][16] f16
    constexpr int NL2 = (B2_IMG + 4095) / 4096;
    constexpr int G_IMG = BM * 64;                                           // one k-tile of G: fp32 [128][16]
    char* W2s = reinterpret_cast<char*>(smem) + G1_BYTES;                    // 2 stages
    // G comes from HBM (the W_o planes from the L2): THREE stages, requested two k-steps ahead - with two, every k-step of GEMM 2 waited
    // out an HBM round trip that had started less than one step before (11.7 ms per launch at 100 samples of L = 352)
    char* Gs = W2s + 2 * B2_IMG;
    // column sums and biases of the gate projection in LDS [2][192] (see gemm3_mlp_block)
    float* cst = reinterpret_cast<float*>(Gs + 3 * G_IMG);
    for (int i = threadIdx.x; i < GT_NG; i += 256) {
        cst[i] = i < g.N ? g.ln_csum[i] : 0.f;
        cst[GT_NG + i] = (i < g.N && g.bias) ? g.bias[i] : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5;
    const int m0 = mt * BM;
    f32x16 acc2[1][TN2];
#pragma unroll
    for (int t = 0; t < TN2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[0][t][r] = 0.f;
    unsigned offs2[NL2];
    plane_sources<BN2, NL2>(g.sB23p, g.sB23n, 0, g.N2, offs2);
    const char* base2 = reinterpret_cast<const char*>(g.B2_split);
    const long long step2 = g.sB23k * 2;
    // G k-tiles: wave w fetches rows 32 w .. 32 w + 31 (two 1 KB chunks of 16 rows), 16-byte slots XOR-swizzled through the source address
    unsigned offsG[2];
    const char* baseG = reinterpret_cast<const char*>(g.gate + (long long)b * g.sGb + (long long)m0 * g.sGm);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (wave * 2 + i) * 16 + (lane >> 2), p = lane & 3;
        const int kq = p ^ ((r >> 2) & 3);
        const int gri = min(m0 + r, g.M - 1) - m0;
        offsG[i] = (unsigned)(((long long)gri * g.sGm + kq * 4) * 4);
    }
    static_assert(B2_IMG % 4096 == 0, "uniform DMA instruction counts per wave (counted waits)");
    auto issue_w2 = [&](int ktile) {                                         // k-tile kt of W_o -> stage kt & 1
        char* dst = W2s + (ktile & 1) * B2_IMG + wave * NL2 * 1024;
        const char* src = base2 + ktile * step2;
#pragma unroll
        for (int i = 0; i < NL2; ++i) glds16(src + vgpr32(offs2[i]), dst + i * 1024);
    };
    const int nkt2 = g.N / 16;                                               // k-tiles of GEMM 2 (N % 16 == 0)
    auto issue_g = [&](int ktile) {                                          // k-tile kt of G -> stage kt % 3; beyond the end: the last one again
        const int kt = min(ktile, nkt2 - 1);                                 // (uniform instruction counts; its stage is not read any more)
        char* dg = Gs + (ktile % 3) * G_IMG + wave * 2048;
        const char* sg = baseG + kt * 64;
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(sg + vgpr32(offsG[i]), dg + i * 1024);
    };
    const int offB2 = plane_off<BN2>(0, lane & 31, h);
    // this lane's 2 x 4 channels of a G k-tile: logical 16-byte slots h and 2 + h of its row
    const int grow = wave * WM + (lane & 31), gx = (grow >> 2) & 3;
    const int offG0 = grow * 64 + ((h ^ gx) << 4), offG1 = grow * 64 + (((2 + h) ^ gx) << 4);
    constexpr int TG2 = 2;
    const bool rows_live = m0 + wave * WM < g.M;

    float ls[1], lq[1], lsh[1] = {0.f};
    float rstd = 0.f, dmean = 0.f;
    constexpr int KC = BN / 16;                                              // k-tiles of GEMM 2 per chunk (6: even, the stage parity runs on)
    const int nchunk = (g.N + BN - 1) / BN;
    for (int c = 0; c < nchunk; ++c) {
        // first W_o k-tile and first TWO G k-tiles of the chunk: they land under GEMM 1 (whose main loop ends with every DMA drained)
        issue_w2(c * KC);
        issue_g(c * KC);
        issue_g(c * KC + 1);
        f32x16 acc1[1][BN / 32];
        if (c == 0) {
            gemm3_mainloop<BM, BN, WM, WN, 0, true, true>(g, smem, mt, c, b, acc1, ls, lq, lsh);
            const float invK = 1.0f / (float)g.K;
            const float sm = ls[0] + __shfl_xor(ls[0], 32, 64), sq = lq[0] + __shfl_xor(lq[0], 32, 64);
            dmean = sm * invK;
            rstd = 1.0f / sqrtf(fmaxf(sq * invK - dmean * dmean, 0.f) + g.ln_eps);
        } else {
            gemm3_mainloop<BM, BN, WM, WN, 0, true, false>(g, smem, mt, c, b, acc1, ls, lq, lsh);
        }
        const int hid0 = c * BN;
#pragma unroll
        for (int j = 0; j < BN / 32; ++j) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int kl = 2 * j + s2;                                   // k-tile of the chunk
                const int kg = c * KC + kl;                                  // k-tile of GEMM 2: W_o stage kg & 1, G stage kg % 3
                // requests of this step, W_o first: the wait at its end leaves the two newest instructions - the G tile - in flight
                if (kl + 1 < KC && (kg + 1) * 16 < g.N) {
                    issue_w2(kg + 1);
                    issue_g(kg + 2);
                }
                u32x4 hf[2];
                {
                    const char* gs = Gs + (kg % 3) * G_IMG;
                    const f32x4 o0 = *reinterpret_cast<const f32x4*>(gs + offG0), o1 = *reinterpret_cast<const f32x4*>(gs + offG1);
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int hc = hid0 + j * 32 + 8 * (2 * s2 + q) + 4 * h;    // 4 consecutive gate channels
                        const int hcl = min(hc, GT_NG - 4);
                        const f32x4 cs = *reinterpret_cast<const f32x4*>(cst + hcl), bi = *reinterpret_cast<const f32x4*>(cst + GT_NG + hcl);
                        const f32x4 ov = q ? o1 : o0;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float x = rstd * (acc1[0][j][8 * s2 + 4 * q + e] - dmean * cs[e]) + bi[e];
                            v[4 * q + e] = (hc + e < g.N) ? ov[e] * sigmoidf_(x) : 0.f;
                        }
                    }
                    // unlifted pieces of v 2^4 (split2b): |gate * o| < 4094, else NaN -> the range probe -> the exact kernels
                    unsigned q0[4], q1[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) split2b(v[2 * e], v[2 * e + 1], q0[e], q1[e]);
                    hf[0] = u32x4{q0[0], q0[1], q0[2], q0[3]};
                    hf[1] = u32x4{q1[0], q1[1], q1[2], q1[3]};
                }
                const char* ws = W2s + (kg & 1) * B2_IMG + offB2;
                if (rows_live && kg * 16 < g.N) {
#pragma unroll
                    for (int t0 = 0; t0 < TN2; t0 += TG2) {
                        u32x4 wb[TG2][2];
#pragma unroll
                        for (int t = 0; t < TG2; ++t)
#pragma unroll
                            for (int p = 0; p < 2; ++p) wb[t][p] = *reinterpret_cast<const u32x4*>(ws + (t0 + t) * 1024 + p * (BN2 * 32));
                        constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};      // smallest first: a1 p0, a0 p1, a0 p0
#pragma unroll
                        for (int term = 0; term < 3; ++term)
#pragma unroll
                            for (int t = 0; t < TG2; ++t)
                                acc2[0][t0 + t] = mfma_split(hf[TA[term]], wb[t][TB[term]], acc2[0][t0 + t]);
                    }
                }
                if (kl + 1 < KC && (kg + 1) * 16 < g.N) wait_vm_and_barrier<2>();
                else wait_vm_and_barrier<0>();                               // last k-tile of the chunk: nothing was requested
            }
        }
    }
    {
        const float cs2 = __builtin_ldexpf(1.0f, -4 - g.b2_exp);
#pragma unroll
        for (int t = 0; t < TN2; ++t) acc2[0][t] *= cs2;
    }
    AbxGemm g2 = g;
    g2.N = g.N2; g2.bias = g.bias2; g2.ln_csum = nullptr; g2.ln_stats = nullptr; g2.act = 0; g2.alpha = 1.0f; g2.gate = nullptr;
    __syncthreads();
    gemm_epilogue<BM, BN2, WM, BN2, EDGE, false>(g2, smem, smem + 2 * BM, acc2, mt * BM, 0, b, false);
}

constexpr int GT_LDS = 2 * 128 * 64 + 2 * 2 * 96 * 32 + 2 * 2 * 192 * 32 + 3 * 128 * 64 + 2 * GT_NG * 4;      // 79 360 bytes (two blocks per CU)

// the round-5 form (two walks over the z rows, one per gate chunk of 96): ABX_TUNE_GTAIL_2WALK, kept for A / B runs and as a cross-check
// (test_gemm_gated_tail_walk_variants_bit_identical)
__global__ __launch_bounds__(256, 2) void gemm3_gtail2w_kernel(const AbxGemm g) {
    extern __shared__ __attribute__((aligned(16))) float gt_smem[];
    const int ntm = (g.M + 127) / 128;
    const unsigned wgid = xcd_contiguous(blockIdx.x, gridDim.x);
    const int b = (int)(wgid / (unsigned)ntm), mt = (int)(wgid - (unsigned)b * (unsigned)ntm);
    const ClockProbe probe(g.clock_probe);
    if ((mt + 1) * 128 <= g.M && g.N2 == 192) gemm3_gtail2w_block<false>(g, gt_smem, mt, b);
    else gemm3_gtail2w_block<true>(g, gt_smem, mt, b);
    probe.finish();
}

// Round 6: ONE walk over the z rows.  The board's power limit holds the clock of every large kernel (profiles/r06a_power_limit.txt), so
// what a launch costs is its energy, and the two-walk form paid the whole A side of GEMM 1 twice: 2 x 98 KB of z rows per block from the
// fabric (the second walk misses the 4 MB L2: 64 resident blocks x 98 KB per XCD), 2 x 12 k-steps of fragment reads, LayerNorm partial
// sums and f16 splits.  Here:
//   GEMM 1   all 192 gate channels in one main loop (128 x 192 tile, swapped operands: gate^T[channel][row], lane = row), 96 accumulator
//            registers - GEMM 2's accumulators do not exist yet;
//   GEMM 2   in two PASSES over the output columns (0 .. 95, then 96 .. 191), 48 accumulator registers each.  Pass A turns the gate
//            accumulators into the operand pieces of sigmoid(gate) * o k-tile by k-tile (the G stream, as before) and KEEPS them (the 96
//            registers the gate accumulators leave); pass B replays them against the other half of W_o.  Each pass streams its half of
//            the W_o planes [2][96][16] per k-tile (the same bytes as one pass over 192 columns), and ends with its own epilogue.
// Every accumulator sees the products of the two-walk form in the same order: bit-identical results.
constexpr int GT1_G1 = 2 * 128 * 64 + 2 * 2 * 192 * 32;                      // stages of GEMM 1: A fp32 + the gate-weight planes, 40 960
constexpr int GT1_W2 = 2 * 96 * 32;                                          // one k-tile of a W_o half: [2][96][16] f16, 6 144
constexpr int GT1_OFF_G = GT1_G1, GT1_OFF_W2 = GT1_OFF_G + 3 * 128 * 64, GT1_OFF_CST = GT1_OFF_W2 + 2 * GT1_W2;
constexpr int GT1_LDS = GT1_OFF_CST + 2 * GT_NG * 4;                         // 79 360 bytes (two blocks per CU)
template <bool EDGE>
__device__ __forceinline__ void gemm3_gtail_block(const AbxGemm& g, float* smem, int mt, int b) {
    constexpr int BM = 128, BN = 192, WM = 32, BH = 96, TH = BH / 32, NKT = BN / 16;
    char* lds = reinterpret_cast<char*>(smem);
    char* Gs = lds + GT1_OFF_G;                                              // 3 stages of G k-tiles (HBM: requested two steps ahead)
    char* W2s = lds + GT1_OFF_W2;                                            // 2 stages; beyond the epilogue's scratch (52 KB from the base)
    float* cst = reinterpret_cast<float*>(lds + GT1_OFF_CST);
    for (int i = threadIdx.x; i < GT_NG; i += 256) {
        cst[i] = i < g.N ? g.ln_csum[i] : 0.f;
        cst[GT_NG + i] = (i < g.N && g.bias) ? g.bias[i] : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5;
    const int m0 = mt * BM;
    // W_o half-tiles: 6 chunks of 1 KB per k-tile - waves 0 .. 2 fetch two each, wave 3 none (its counted waits below only ever leave the
    // G pair in flight, which is the newest pair of every wave)
    unsigned offs2[2][2];
#pragma unroll
    for (int half = 0; half < 2; ++half) plane_sources<BH, 2>(g.sB23p, g.sB23n, half * BH, g.N2, offs2[half]);
    const char* base2 = reinterpret_cast<const char*>(g.B2_split);
    const long long step2 = g.sB23k * 2;
    auto issue_w2 = [&](int half, int ktile) {                               // k-tile kt of the W_o half -> stage kt & 1
        if (wave == 3) return;
        char* dst = W2s + (ktile & 1) * GT1_W2 + wave * 2048;
        const char* src = base2 + ktile * step2;
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(src + vgpr32(offs2[half][i]), dst + i * 1024);
    };
    unsigned offsG[2];
    const char* baseG = reinterpret_cast<const char*>(g.gate + (long long)b * g.sGb + (long long)m0 * g.sGm);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (wave * 2 + i) * 16 + (lane >> 2), p = lane & 3;
        const int kq = p ^ ((r >> 2) & 3);
        const int gri = min(m0 + r, g.M - 1) - m0;
        offsG[i] = (unsigned)(((long long)gri * g.sGm + kq * 4) * 4);
    }
    const int nkt2 = g.N / 16;                                               // k-tiles of GEMM 2 (N % 16 == 0; <= NKT)
    auto issue_g = [&](int ktile) {                                          // k-tile kt of G -> stage kt % 3; beyond the end: the last one again
        const int kt = min(ktile, nkt2 - 1);
        char* dg = Gs + (ktile % 3) * (BM * 64) + wave * 2048;
        const char* sg = baseG + kt * 64;
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(sg + vgpr32(offsG[i]), dg + i * 1024);
    };
    const int offB2 = plane_off<BH>(0, lane & 31, h);
    const int grow = wave * WM + (lane & 31), gx = (grow >> 2) & 3;
    const int offG0 = grow * 64 + ((h ^ gx) << 4), offG1 = grow * 64 + (((2 + h) ^ gx) << 4);
    const bool rows_live = m0 + wave * WM < g.M;

    // ---- GEMM 1: gate^T for all gate channels; the first W_o half-tile and the first two G k-tiles land under it
    issue_w2(0, 0);
    issue_g(0);
    issue_g(1);
    float ls[1], lq[1], lsh[1] = {0.f};
    f32x16 acc1[1][BN / 32];
    gemm3_mainloop<BM, BN, WM, BN, 0, true, true>(g, smem, mt, 0, b, acc1, ls, lq, lsh);
    const float invK = 1.0f / (float)g.K;
    const float sm = ls[0] + __shfl_xor(ls[0], 32, 64), sq = lq[0] + __shfl_xor(lq[0], 32, 64);
    const float dmean = sm * invK;
    const float rstd = 1.0f / sqrtf(fmaxf(sq * invK - dmean * dmean, 0.f) + g.ln_eps);

    AbxGemm g2 = g;
    g2.N = g.N2; g2.bias = g.bias2; g2.ln_csum = nullptr; g2.ln_stats = nullptr; g2.act = 0; g2.alpha = 1.0f; g2.gate = nullptr;
    const float cs2 = __builtin_ldexpf(1.0f, -4 - g.b2_exp);
    u32x4 hfa[NKT][2];                                                       // the pieces of sigmoid(gate) * o, k-tile by k-tile (pass A -> pass B)
    constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};                      // smallest first: a1 p0, a0 p1, a0 p0
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        f32x16 acc2[1][TH];
#pragma unroll
        for (int t = 0; t < TH; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[0][t][r] = 0.f;
        if (half == 1) issue_w2(1, 0);                                       // (requested after the barrier that ended pass A's last step)
#pragma unroll
        for (int kg = 0; kg < NKT; ++kg) {
            const bool more = (kg + 1) * 16 < g.N && kg + 1 < NKT;
            if (half == 1 && kg == 0) wait_vm_and_barrier<0>();               // pass B's first half-tile has landed
            // requests of this step, W_o first: the wait at its end leaves the two newest instructions - the G tile - in flight
            if (more) {
                issue_w2(half, kg + 1);
                if (half == 0) issue_g(kg + 2);
            }
            if (half == 0) {
                const int j = kg >> 1, s2 = kg & 1;
                const char* gs = Gs + (kg % 3) * (BM * 64);
                const f32x4 o0 = *reinterpret_cast<const f32x4*>(gs + offG0), o1 = *reinterpret_cast<const f32x4*>(gs + offG1);
                float v[8];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int hc = j * 32 + 8 * (2 * s2 + q) + 4 * h;        // 4 consecutive gate channels
                    const int hcl = min(hc, GT_NG - 4);
                    const f32x4 cs = *reinterpret_cast<const f32x4*>(cst + hcl), bi = *reinterpret_cast<const f32x4*>(cst + GT_NG + hcl);
                    const f32x4 ov = q ? o1 : o0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x = rstd * (acc1[0][j][8 * s2 + 4 * q + e] - dmean * cs[e]) + bi[e];
                        v[4 * q + e] = (hc + e < g.N) ? ov[e] * sigmoidf_(x) : 0.f;
                    }
                }
                // unlifted pieces of v 2^4 (split2b): |gate * o| < 4094, else NaN -> the range probe -> the exact kernels
                unsigned q0[4], q1[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) split2b(v[2 * e], v[2 * e + 1], q0[e], q1[e]);
                hfa[kg][0] = u32x4{q0[0], q0[1], q0[2], q0[3]};
                hfa[kg][1] = u32x4{q1[0], q1[1], q1[2], q1[3]};
            }
            const char* ws = W2s + (kg & 1) * GT1_W2 + offB2;
            if (rows_live && kg * 16 < g.N) {
                u32x4 wb[TH][2];
#pragma unroll
                for (int t = 0; t < TH; ++t)
#pragma unroll
                    for (int p = 0; p < 2; ++p) wb[t][p] = *reinterpret_cast<const u32x4*>(ws + t * 1024 + p * (BH * 32));
#pragma unroll
                for (int term = 0; term < 3; ++term)
#pragma unroll
                    for (int t = 0; t < TH; ++t) acc2[0][t] = mfma_split(hfa[kg][TA[term]], wb[t][TB[term]], acc2[0][t]);
            }
            if (more && half == 0) wait_vm_and_barrier<2>();
            else wait_vm_and_barrier<0>();                                   // (pass B, or the last k-tile: nothing but W_o was requested)
        }
#pragma unroll
        for (int t = 0; t < TH; ++t) acc2[0][t] *= cs2;
        // (every DMA has landed and every wave is past its last stage read: the scratch of the epilogue overlays the GEMM 1 stages and
        // the head of the G ring, not the W_o stages - pass B's first half-tile is requested above, after this epilogue)
        gemm_epilogue<BM, BH, WM, BH, EDGE, false>(g2, smem, smem + 2 * BM, acc2, m0, half * BH, b, false);
        if (half == 0) __syncthreads();
    }
}

__global__ __launch_bounds__(256, 2) void gemm3_gtail_kernel(const AbxGemm g) {
    extern __shared__ __attribute__((aligned(16))) float gt_smem[];
    const int ntm = (g.M + 127) / 128;
    const unsigned wgid = xcd_contiguous(blockIdx.x, gridDim.x);
    const int b = (int)(wgid / (unsigned)ntm), mt = (int)(wgid - (unsigned)b * (unsigned)ntm);
    const ClockProbe probe(g.clock_probe);
    if ((mt + 1) * 128 <= g.M && g.N2 == 192 && g.N == 192) gemm3_gtail_block<false>(g, gt_smem, mt, b);
    else gemm3_gtail_block<true>(g, gt_smem, mt, b);
    probe.finish();
}


template <int BM, int BN, int WM, int WN, int MINW>
int launch3(const AbxGemm& g, hipStream_t st, AbxPlan* plan) {
    const long long mt = ((long long)g.M + BM - 1) / BM, ntn = ((long long)g.N + BN - 1) / BN;
    dim3 grid((unsigned)(mt * ntn * g.batch), 1, 1), block(256);
    const int amode = g.A_split ? 2 : (g.sAk == 1 ? 0 : 1);
#define GEMM3_LAUNCH(AMODE, TS)                                                                                         \
    ABX_LAUNCH(plan, ("gemm3_kernel<%d, %d, %d, %d, %d, %s, %d>", BM, BN, WM, WN, AMODE, ABX_BOOL(TS), MINW), "abx_gemm", \
               (gemm3_kernel<BM, BN, WM, WN, AMODE, TS, MINW>), 0, grid, block, 0, st, g)
    if (g.c_transposed) {
        if (amode != 0) { abx_set_error("abx_gemm: transposed store needs a k-contiguous fp32 A"); return ABX_ERR_ARG; }
        return GEMM3_LAUNCH(0, true);
    }
    if (amode == 0) return GEMM3_LAUNCH(0, false);
    if (amode == 1) return GEMM3_LAUNCH(1, false);
    return GEMM3_LAUNCH(2, false);
#undef GEMM3_LAUNCH
}

// fp32 weights -> k-tiled float16 planes [Kp/16][2][N][16] of w' = w * scale: p0 = f16(w'), p1 = f16(w' - p0) (AbxGemm.b_f16)
__global__ __launch_bounds__(256) void split_weights_f16_kernel(const float* __restrict__ w, long long s_n, long long s_k, int N, int K,
                                                                int Kp, float scale, unsigned short* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)N * Kp) return;
    const int n = (int)(idx / Kp), k = (int)(idx % Kp);
    const float x = k < K ? w[n * s_n + k * s_k] * scale : 0.f;
    const _Float16 h0 = (_Float16)x;
    const _Float16 h1 = (_Float16)(x - (float)h0);
    const long long o = ((long long)(k >> 4) * 2 * N + n) * 16 + (k & 15);
    out[o] = __builtin_bit_cast(unsigned short, h0);
    out[o + (long long)N * 16] = __builtin_bit_cast(unsigned short, h1);
}

}  // namespace

// Called by abx_gemm (gemm.hip) once the descriptor has been validated and the vector flags filled.
// Returns 1 when the problem is not served by this path (the caller falls back to the exact kernel).
int abx_gemm3_dispatch(const AbxGemm& g, hipStream_t st, int* rc, AbxPlan* plan) {
    // N <= 32 with split weights: the skinny projections of the pair stack (4 / 12 / 32 bias channels from 192- / 128-wide rows):
    // HBM streams of the A operand, served by a 128 x 32 tile of the same DMA pipeline (7 blocks per CU keep the stream fed)
    const bool narrow = g.B_split && g.N <= 32 && !g.A_split && g.sAk == 1 && !g.glu && !g.C_split && !g.A2 && !g.out_ln_w &&
                        g.a_pair_transpose <= 0 && g.pair_Lp == 0;
    // (N <= 64 with weight planes goes to the exact kernel; a plane x plane product has no fp32 operands to fall back on and stays here at
    // any N: the tri-mul contraction of a complex of exactly 64 residues is M = N = 64)
    if (!g.B_split || g.K % 16 != 0 || (g.N <= 64 && !narrow && !g.A_split)) return 1;
    if ((g.A_split != nullptr) == (g.b_f16 != 0) || !exp_ok(g.b_exp) || !exp_ok(g.b2_exp)) {
        abx_set_error("abx_gemm: B_split must be float16 weight planes (abx_split_weights_f16, b_f16 = 1, |b_exp| <= 100) with an fp32 A "
                      "and activation images (b_f16 = 0) with A_split");
        *rc = ABX_ERR_ARG;
        return 0;
    }
    const long long mt128 = ((long long)g.M + 127) / 128;
    // exact == 2: the caller fixed the arithmetic class of this op (results must not depend on how many samples share a launch)
    if (g.exact != 2 && mt128 * (((long long)g.N + 127) / 128) * g.batch < ABX_SPLIT_MIN_TILES) return 1;
    if (!planes_ok(g.B_split, g.sB3n, g.sB3p, g.sB3k, g.sB3b)) return 1;
    if (g.A_split) {
        if (!planes_ok(g.A_split, g.sA3m, g.sA3p, g.sA3k, g.sA3b) || g.c_transposed) return 1;
        if (g.batch_inner > 0 && (g.sA3i % 8 != 0 || g.sB3i % 8 != 0)) return 1;
    } else if (g.sAk == 1) {
        if (!rows_ok(g.A, g.sAm, g.sAb)) return 1;
        if (g.a_pair_transpose > 0 && !g.a_pair && (long long)g.a_pair_transpose * g.a_pair_transpose != g.M) return 1;
    } else {
        if (!rows_ok(g.A, g.sAk, g.sAb) || g.M % 4 != 0 || g.M < 4 || g.a_pair_transpose > 0) return 1;
    }
    // 128x128 tiles run 3 blocks per CU (48 KB LDS, ~150 VGPRs), 128x192 tiles 2: the narrow tile wins whenever it wastes no
    // columns (N = 768: q|k|v|gate, transition hidden); N = 192 / 448 take the wide tile
    // per-lane DMA offsets are 32-bit, relative to the tile's first row (k-contiguous A), to the batch base (pair-transposed
    // rows, plane operands) or to the tile's first column (row-contiguous A)
    if (!g.A_split && g.sAk == 1 && ((g.a_pair_transpose > 0 || g.a_pair) ? (long long)g.M * g.sAm : 128LL * g.sAm) >= (1LL << 30)) return 1;
    if (g.pair_Lp > 0 && g.c_pair && g.c_transposed) return 1;
    if (g.a_pair && (g.A_split || g.sAk != 1)) return 1;
    if (!g.A_split && g.sAk != 1 && 16LL * g.sAk + g.M >= (1LL << 30)) return 1;
    if (((long long)g.M + 127) / 128 * (((long long)g.N + 127) / 128) * g.batch >= (1LL << 31)) return 1;
    if (g.A_split && (long long)(g.K / 16) * g.sA3k >= (1LL << 31)) return 1;
    if ((long long)(g.K / 16) * g.sB3k >= (1LL << 31)) return 1;
    if (g.out_ln_w) {
        if (g.N > 128 || g.c_transposed || g.C_split || g.A2 || g.A_split || g.sAk != 1 || !g.out_ln_b) {
            abx_set_error("abx_gemm: out_ln needs N <= 128, a k-contiguous fp32 A and a plain store (split-f16 path)");
            *rc = ABX_ERR_ARG;
            return 0;
        }
        const long long mt = ((long long)g.M + 127) / 128;
        *rc = ABX_LAUNCH_LIT(plan, "abx_gemm(out_ln)", (gemm3_oln_kernel<128, 128, 32, 128, 4>), 0, dim3((unsigned)(mt * g.batch)), dim3(256), 0, st, g);
        return 0;
    }
    if (g.mlp == 2) {
        // gated attention tail: out = (sigmoid(LN(A) B + bias) * gate) B2 + bias2 (+ resid)
        if (g.A_split || g.sAk != 1 || g.c_transposed || g.C_split || g.glu || g.A2 || g.out_ln_w || !g.B2_split || g.N2 <= 0 || g.N2 > 192 ||
            g.N % 16 != 0 || g.N > GT_NG || g.act != 2 || g.alpha != 1.0f || g.rowscale || !g.gate || !g.ln_csum || g.ln_stats || g.a_relu ||
            g.a_pair_transpose > 0 || g.pair_Lp > 0 || !planes_ok(g.B2_split, g.sB23n, g.sB23p, g.sB23k) ||
            (long long)(g.N / 16) * g.sB23k >= (1LL << 31) || !al16(g.ln_csum) || (g.bias && !al16(g.bias)) || !rows_ok(g.gate, g.sGm, g.sGb) ||
            128LL * g.sGm >= (1LL << 30)) {
            abx_set_error("abx_gemm: mlp = 2 (gated tail) needs a k-contiguous fp32 A with folded LayerNorm, act = 2, a 16-byte aligned gate "
                          "operand [M][N], N % 16 == 0, N2 <= 192, plain store, B2_split planes in the permuted k order");
            *rc = ABX_ERR_ARG;
            return 0;
        }
        const long long mt = ((long long)g.M + 127) / 128;
        const dim3 grid((unsigned)(mt * g.batch)), block(256);
        if (g.tune & ABX_TUNE_GTAIL_2WALK)                                   // the two-walk form of round 5 (A / B runs, cross-check)
            *rc = ABX_LAUNCH_LIT(plan, "abx_gemm(gated tail, two walks)", &gemm3_gtail2w_kernel, GT_LDS, grid, block, GT_LDS, st, g);
        else
            *rc = ABX_LAUNCH_LIT(plan, "abx_gemm(gated tail)", &gemm3_gtail_kernel, GT1_LDS, grid, block, GT1_LDS, st, g);
        return 0;
    }
    if (g.mlp) {
        // fused two-layer transition: hidden = relu(LN(A) B + bias) never stored, out = hidden B2 + bias2 (+ resid)
        if (g.A_split || g.sAk != 1 || g.c_transposed || g.C_split || g.glu || g.A2 || g.out_ln_w || !g.B2_split || g.N2 <= 0 || g.N2 > 192 ||
            g.N % 16 != 0 || g.N > MLP_NH || g.act != 1 || g.alpha != 1.0f || g.rowscale || g.gate || !g.ln_csum || g.ln_stats || g.a_relu ||
            g.a_pair_transpose > 0 || g.pair_Lp > 0 || !planes_ok(g.B2_split, g.sB23n, g.sB23p, g.sB23k) ||
            (long long)(g.N / 16) * g.sB23k >= (1LL << 31) || !al16(g.ln_csum) || (g.bias && !al16(g.bias))) {
            abx_set_error("abx_gemm: mlp needs a k-contiguous fp32 A with folded LayerNorm, relu, N % 16 == 0, N <= 768, N2 <= 192, plain store, "
                          "B2_split planes in the permuted k order");
            *rc = ABX_ERR_ARG;
            return 0;
        }
        const long long mt = ((long long)g.M + 127) / 128;
        const dim3 grid((unsigned)(mt * g.batch)), block(256);
        // RETIRED, kept compiled: gemm_prepare refuses ABX_TUNE_MLP_MINB1 (and NARROW_RING below, FORCE in gemm.hip), so these branches are never
        // taken.  They stay because they instantiate kernels whose removal changes the machine code of kernels that stay, which share helper
        // functions with them ("Retired GEMM variants").  Take them out together with a measurement of those kernels.
        if (g.tune & ABX_TUNE_MLP_MINB1) *rc = ABX_LAUNCH_LIT(plan, "abx_gemm(mlp)", &gemm3_mlp_kernel<1>, 0, grid, block, 0, st, g);         // (retired, unreachable: see below)
        else *rc = ABX_LAUNCH_LIT(plan, "abx_gemm(mlp)", &gemm3_mlp_kernel<2>, 0, grid, block, 0, st, g);
        return 0;
    }
    if (g.A2) {
        // dual GEMM: 128 x 96 tiles (two accumulator sets of 48 registers)
        if (g.A_split || g.c_transposed || g.glu || !g.B2_split || g.K2 % 16 != 0 || !rows_ok(g.A2, g.sA2m, g.sA2b) ||
            !planes_ok(g.B2_split, g.sB23n, g.sB23p, g.sB23k) || !g.ln2_csum ||
            (g.pair_Lp > 0 ? (long long)g.pair_L * g.pair_L * g.sA2m : 128LL * g.sA2m) >= (1LL << 30) ||
            (long long)(g.K2 / 16) * g.sB23k >= (1LL << 31)) {
            abx_set_error("abx_gemm: dual (A2 / B2_split) operands do not qualify for the split-f16 dual kernel");
            *rc = ABX_ERR_ARG;
            return 0;
        }
        // (128 x 192 tiles - A read and split once per row - need 2 x 96 accumulator registers and spill at 256 VGPRs)
        const long long mt = ((long long)g.M + 127) / 128, ntn = ((long long)g.N + 95) / 96;
        // Three blocks per CU (142 VGPRs).  ABX_TUNE_DUAL_1WALK (96 < N <= 192): one block per row tile, z walked once (gemm3_dual1_kernel),
        // the bit-identical cross-check of the default
        const dim3 grid((unsigned)(mt * ntn * g.batch)), block(256);
        if (g.N > 96 && g.N <= 192 && (g.tune & ABX_TUNE_DUAL_1WALK)) *rc = ABX_LAUNCH_LIT(plan, "abx_gemm(dual)", &gemm3_dual1_kernel, 0, dim3((unsigned)(mt * g.batch)), block, 0, st, g);
        else *rc = ABX_LAUNCH_LIT(plan, "abx_gemm(dual)", (gemm3_dual_kernel<128, 96, 32, 96, 3>), 0, grid, block, 0, st, g);
        return 0;
    }
    if (narrow) {
        const long long mt = ((long long)g.M + 127) / 128;
        dim3 grid((unsigned)(mt * g.batch), 1, 1), block(256);
        if (const int v = (g.tune & ABX_TUNE_NARROW_RING_MASK) >> ABX_TUNE_NARROW_RING_SHIFT) {      // (retired, unreachable: see the fused transition above)
            const char* what = "abx_gemm(narrow, ring)";
            if (g.c_transposed && v == 1) *rc = ABX_LAUNCH_LIT(plan, what, (gemm3_narrow_ring_kernel<true, 3, 4>), 0, grid, block, 0, st, g);
            else if (g.c_transposed) *rc = ABX_LAUNCH_LIT(plan, what, (gemm3_narrow_ring_kernel<true, 4, 3>), 0, grid, block, 0, st, g);
            else if (v == 1) *rc = ABX_LAUNCH_LIT(plan, what, (gemm3_narrow_ring_kernel<false, 3, 4>), 0, grid, block, 0, st, g);
            else *rc = ABX_LAUNCH_LIT(plan, what, (gemm3_narrow_ring_kernel<false, 4, 3>), 0, grid, block, 0, st, g);
            return 0;
        }
        if (g.c_transposed) *rc = ABX_LAUNCH_LIT(plan, "abx_gemm(narrow)", (gemm3_kernel<128, 32, 32, 32, 0, true, 6>), 0, grid, block, 0, st, g);
        else *rc = ABX_LAUNCH_LIT(plan, "abx_gemm(narrow)", (gemm3_kernel<128, 32, 32, 32, 0, false, 6>), 0, grid, block, 0, st, g);
        return 0;
    }
    const long long pad128 = ((g.N + 127) / 128) * 128, pad192 = ((g.N + 191) / 192) * 192;
    // (the plane x plane contraction at L = 352 pads to 384 either way: the wide tile measured 10 % faster)
    const bool wide = g.glu ? false : (g.A_split ? pad192 <= pad128 : (pad192 <= pad128 && g.N % 128 != 0));
    // waves are stacked along M (4 x 1): every wave owns 32 rows and the full tile width, so each A row is read from LDS and
    // split into f16 pieces by exactly one wave (the VALU issue slots next to the MFMAs are the scarce resource)
    // Small problems (the per-residue GEMMs of the IPA loop / sequence track at a dozen samples per GPU: 4 224 rows x 256 columns = 66
    // tiles of 128 x 128 on 256 CUs): 64 x 128 tiles, 2 x 2 waves, twice the workgroups.  Every output element still accumulates its k
    // in the same order (same MFMA, same term order, same row statistics), so the tile choice does not change a single bit and
    // results stay independent of how many samples share a launch.
    const long long ntn128 = ((long long)g.N + 127) / 128;
    if (!wide && !g.glu && mt128 * ntn128 * g.batch < 384 && g.M > 64) *rc = launch3<64, 128, 32, 64, 4>(g, st, plan);
    else if (wide) *rc = launch3<128, 192, 32, 192, 3>(g, st, plan);
    else *rc = launch3<128, 128, 32, 128, 4>(g, st, plan);
    return 0;
}

// abx_gemm_side (gemm.hip): both descriptors validated and their vector flags filled.  Returns 1 when the pair is not served by
// the side kernel (the caller then issues two launches).
int abx_gemm3_side_dispatch(const AbxGemm& g, const AbxGemm& s2, hipStream_t st, int* rc, AbxPlan* plan) {
    auto plain_a = [&](const AbxGemm& d) {
        return d.B_split && d.b_f16 && !d.A_split && d.A && d.sAk == 1 && d.K % 16 == 0 && rows_ok(d.A, d.sAm, d.sAb) &&
               planes_ok(d.B_split, d.sB3n, d.sB3p, d.sB3k, d.sB3b) && exp_ok(d.b_exp) &&
               !d.glu && !d.C_split && !d.A2 && !d.out_ln_w && !d.mlp && d.a_pair_transpose <= 0 && d.pair_Lp == 0 && d.batch_inner == 0 &&
               128LL * d.sAm < (1LL << 30) && (long long)(d.K / 16) * d.sB3k < (1LL << 31) && d.exact != 1;
    };
    if (!plain_a(g) || !plain_a(s2)) return 1;
    if (g.c_transposed || g.N % 128 != 0 || g.N < 128) return 1;                      // main: the 128 x 128 plain-store kernel
    if (!s2.c_transposed || s2.N > 32) return 1;                                      // side: the 128 x 32 transposed-store tile
    const long long tq = ((long long)g.M + 127) / 128 * (g.N / 128) * g.batch, ts = ((long long)s2.M + 127) / 128 * s2.batch;
    if (tq < 384 || ts <= 0 || ts > tq || tq + ts >= (1LL << 31)) return 1;           // (small problems keep their own tile choice)
    *rc = ABX_LAUNCH_LIT(plan, "abx_gemm_side", &gemm3_side_kernel, 0, dim3((unsigned)(tq + ts)), dim3(256), 0, st, g, s2);
    return 0;
}

// resident workgroups per CU of the main instantiations (diagnostics for tools/kbench.py)
extern "C" int abx_gemm3_occupancy(int which) {
    int n = -1;
    hipError_t e = hipErrorInvalidValue;
    if (which == 0) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(&gemm3_kernel<128, 192, 32, 192, 0, false, 3>), 256, 0);
    else if (which == 1) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(&gemm3_kernel<128, 128, 32, 128, 0, false, 4>), 256, 0);
    else if (which == 2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(&gemm3_kernel<128, 128, 32, 128, 0, true, 4>), 256, 0);
    else if (which == 3) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(&gemm3_kernel<128, 192, 32, 192, 2, false, 3>), 256, 0);
    return e == hipSuccess ? n : -(int)e - 1000;
}

extern "C" int abx_split_weights_f16(const float* w, long long s_n, long long s_k, int N, int K, int scale_exp, unsigned short* out,
                                     hipStream_t st) {
    ABX_REQUIRE(w && out && N > 0 && K > 0 && scale_exp >= -100 && scale_exp <= 100, "abx_split_weights_f16: bad args");
    const int Kp = (K + 15) / 16 * 16;
    const long long total = (long long)N * Kp;
    hipLaunchKernelGGL(split_weights_f16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, s_n, s_k, N, K, Kp,
                       ldexpf(1.0f, scale_exp), out);
    return abx_check_launch("abx_split_weights_f16");
}
