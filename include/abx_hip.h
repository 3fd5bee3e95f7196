/* libabx_hip — C ABI of the MI355X (gfx950) kernels behind AbX's reverse-diffusion sampling hot path.
 *
 * The reference (CarbonMatrixLab/AbX) is pure PyTorch: it has no FFI of its own, so the "binding" a maintainer
 * adds is a ctypes stub that replaces the ATen op groups listed in SURVEY.md §2.1 / §8(a).
 * Every entry below cites the reference site (file:line under the reference root) it replaces.
 *
 * Conventions:
 *   - raw DEVICE pointers + explicit sizes/strides (in ELEMENTS) + hipStream_t; no torch types;
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library keeps no mutable global state;
 *   - every entry returns int: 0 = ok, <0 = argument check failed, >0 = hipError_t of the launch;
 *     abx_last_error_string() gives the thread-local message;
 *   - asynchronous on the given stream, no internal synchronisation (hipGraph-capturable), re-entrant.
 */
#ifndef ABX_HIP_H
#define ABX_HIP_H

#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
typedef struct ihipStream_t* hipStream_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ABX_HIP_ABI_VERSION 1

int abx_version(void);
const char* abx_last_error_string(void);
/* device properties sanity check: returns 0 when the current device is gfx950 */
int abx_init(int device);
/* diagnostics: fill the LDS of every CU with `pattern` (results must not depend on stale LDS contents) */
int abx_debug_poison_lds(unsigned pattern, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Dense contractions.  Replaces every torch Linear / LayerNorm->Linear / einsum on the path:
 * abx/model/common_modules.py:11-44 (Linear), abx/model/seqformer.py:358-376 (Transition), :380-411 (OPM out_proj),
 * :443-504 (TriangleMultiplication projections + 'bikc,bjkc->bijc' / 'bkic,bkjc->bijc'), :260-312 (q/k/v/gate/out),
 * abx/model/score_network.py:117-137, abx/model/folding.py:69-132 (IPA projections), abx/model/head.py:147-160,207-220.
 *   acc[b][m][n] = sum_k relu?(A[b][m][k]) * B[b][k][n]
 *   LayerNorm over k is applied algebraically in the epilogue: pass B scaled by gamma (B[k][n] = gamma[k] W[n][k]),
 *   ln_csum[n] = sum_k B[k][n], bias[n] = sum_k beta[k] W[n][k] + b[n] and the row statistics:  ln(v) = rstd[m] (v - mean[m] csum[n])
 *   epi(v) = ((ln(v) + bias[n]) * alpha) -> act -> * rowscale[b][m] -> * (sigmoid?)(gate[b][m][n]) -> + resid[b][m][n]
 *
 * MODES.  Beside the plain GEMM the descriptor selects one of the fused forms below; abx_gemm_check_modes (called by abx_gemm first,
 * callable on its own without a GPU) rejects every pair marked x with a negative code and a message that names both modes.
 *   glu       glu = 1: (value, gate) column pairs -> value * sigmoid(gate)             (tri-mul projections, seqformer.py:480-485)
 *   mlp       mlp = 1 + B2_split: relu(LN(A) B + b) B2 + b2 (+ resid), hidden on-chip   (pair Transition, seqformer.py:358-376)
 *   dual      A2 + B2_split: epi(A B) * sigmoid(LN(A2) B2 + b2) (+ resid)               (tri-mul tail, seqformer.py:496-503)
 *   c_split   C_split: output as the f16 operand image of the following contraction     (tri-mul projections)
 *   out_ln    out_ln_w: LayerNorm over the OUTPUT row                                    (IpaScore pair init, score_network.py:117-120)
 *   a_split   A_split (+ B_split of activations): plane x plane contraction             ('bikc,bjkc->bijc', seqformer.py:490-493)
 *   pair      pair_Lp > 0 / a_pair / c_pair / a_pair_transpose: padded or transposed pair-row maps
 *   exact     exact = 1: the exact fp32-MFMA kernels (plain epilogue only)
 *
 *              glu   mlp   dual  c_split out_ln a_split pair  exact
 *   glu         .     x     x     ok      x      x      ok    x
 *   mlp         x     .     x     x       x      x      x     x
 *   dual        x     x     .     x       x      x      ok    x
 *   c_split     ok    x     x     .       x      x      ok    x
 *   out_ln      x     x     x     x       .      x      x     x
 *   a_split     x     x     x     x       x      .      x     x
 *   pair        ok    x     ok    ok      x      x      .     x
 *   exact       x     x     x     x       x      x      x     .
 * Further requirements of a single mode (also checked, same function): glu and c_split need c_transposed; glu: N % 128 == 0, no gate;
 * mlp: act = 1, folded LayerNorm (ln_csum, no ln_stats), N2 <= 192, no gate / rowscale / c_transposed; dual: ln2_csum, no c_transposed;
 * out_ln: N <= 128, out_ln_b, no c_transposed; a_split: no LayerNorm, no a_relu (there is no fp32 row to normalise).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct AbxGemm {
    const float* A; long long sAb, sAm, sAk;       /* one of sAm / sAk must be 1 */
    const float* B; long long sBb, sBk, sBn;       /* one of sBk / sBn must be 1 */
    float* C;       long long sCb, sCm;            /* n-contiguous; if c_transposed: (m,n) at C + b*sCb + n*sCm + m */
    int M, N, K, batch;
    int c_transposed;
    const float* ln_stats; long long sSb;          /* (mean,rstd) pairs, row index b*sSb + m; NULL with ln_csum set = the kernel
                                                      computes the row statistics itself from the A operand stream */
    const float* ln_csum;                          /* [N] column sums of the gamma-scaled B; NULL = no LayerNorm */
    float ln_eps;                                  /* inline statistics: epsilon (0 -> 1e-5) */
    int a_relu;
    const float* bias;                             /* [N] or NULL */
    float alpha;                                   /* use 1.0f for none */
    int act;                                       /* 0 none, 1 relu, 2 sigmoid */
    const float* rowscale; long long sRSb;         /* [b*sRSb + m] or NULL */
    const float* gate; long long sGb, sGm; int gate_sigmoid;   /* addressed like C: (m,n) at gate + b*sGb + m*sGm + n, or */
    const float* resid; long long sRb, sRm;        /* + n*sGm + m when c_transposed; resid likewise and may alias C */
    /* Split-f16 operands and output (csrc/gemm3.hip): every fp32 product of the large contractions is evaluated on the float16
     * matrix cores (v_mfma_f32_32x32x16_f16, fp32 accumulate) from 3 exact partial products:
     *     x y  ~  a1 p2 + a0 p1 + a0 p0      A side (two pieces):  x' = x 2^-4,  a0 = f16(x'),  a1 = f16((x' - a0) 2^11)
     *                                        B side (two planes):   y' = y 2^e,   p0 = f16(y'),  p1 = f16(y' - p0);  p2 = f16(p0 2^-11)
 *                                                               is derived in registers (one rounding of an exact value)
     * A piece pair carries 23 significant bits (|x' - a0 - a1 2^-11| <= 2^-23 |x'| worst case, 2^-25 on average), the dropped term
     * a1 p1 2^-11 is <= 2^-22 |x y| with mean zero: measured as accurate as the exact fp32 MFMA kernel
     * (tests/test_gpu_kernels.py::test_gemm_split_accuracy_vs_exact).  A-side range: |x| < 2^20, full relative precision from
     * |x| = 2^-9, 2^-32 absolute below; an operand beyond the range becomes inf - inf = NaN in its output row, never a silently wrong
     * number (remedy: exact = 1).  fp32 A operands are split in registers by the kernels.
     *   Weights (B of an fp32-A GEMM): abx_split_weights_f16 planes with a per-tensor e = b_exp (max |y'| in [2^13, 2^14)): b_f16 = 1;
     *     the accumulators are multiplied by 2^(4 - b_exp) before the epilogue.
     *   Activations on both sides (A_split and B_split: the TriangleMultiplication contraction): images written by the C_split
     *     epilogue of the projection GEMM, B side with the fixed e = 4 (|y| < 4095; 2^-29 absolute below 2^-6); b_f16 = 0.
     * The planes are k-TILED: element (row, k) of plane p at base + batch*sXb + (k/16)*sXk + p*sXp + row*sXr + k%16 (16-bit units),
     * i.e. the 16 k of one k-tile are contiguous (abx_split_weights_f16 writes [Kp/16][2][N][16]: sB3k = 2*N*16, sB3p = N*16,
     * sB3n = 16). */
    const unsigned short* B_split; long long sB3p, sB3n, sB3k, sB3b;   /* B as planes (sB3b = 0: shared weights); used instead of B */
    const unsigned short* A_split; long long sA3p, sA3m, sA3k, sA3b;   /* A as planes (pieces a0, a1), used instead of A:
                                                      the TriangleMultiplication contraction takes both operands this way (K % 16 == 0) */
    int batch_inner; long long sA3i, sB3i;         /* batch_inner > 0: two-level batch of the plane operands, entry b sits at
                                                      (b / batch_inner) * sX3b + (b % batch_inner) * sX3i (left / right channels of
                                                      one sample inside a wider channel tensor) */
    int c_split_tile;                              /* with C_split, pair_Lp > 0 and a_pair: the M = ceil8(pair_L) * ceil16(pair_Lp) GEMM rows are
                                                      pair positions (i, k) in blocks of (8 i x 16 k), m = ((i/8) * KT + k/16) * 128 + (i%8) * 16
                                                      + k%16 (KT = ceil(pair_Lp / 16)): 64 contiguous plane bytes per store instruction and
                                                      channel.  rowscale stays indexed [i * pair_Lp + k] */
    int c_split_nA;                                /* with C_split: output channels n < c_split_nA are written as the A side of the
                                                      following contraction (pieces a0, a1), the others as its B side (planes p0, p1): two planes per channel */
    unsigned short* C_split; long long sCp, sCk; int c_split_L;   /* write the output as planes instead of C, laid out as the
                                                      k-tiled OPERAND of the following contraction: with m = i*L + k (L =
                                                      c_split_L, M % L == 0, transposed store only), element (m, n) of plane p goes to
                                                      C_split + b*sCb + n*sCm + (k/16)*sCk + p*sCp + i*16 + k%16 */
    int glu;                                       /* transposed store only: the N columns are (value, gate) pairs of 32-column blocks
                                                      [v0 | g0 | v1 | g1 | ...] of the same N/2 output channels (weights packed that
                                                      way); out = epi(value) * sigmoid(epi(gate)), C / C_split have N/2 channels.
                                                      Needs a kernel whose wave tile holds both blocks (split-f16 128x128 tiles) */
    int a_pair_transpose;                          /* L > 0: M == L*L rows per batch are pair positions (i,k); row i*L + k of
                                                      the GEMM reads source row k*L + i (k-contiguous A, split-f16 path only) */
    int pair_L, pair_Lp;                           /* pair_Lp > 0: the M rows of the GEMM are PADDED pair positions m = i*pair_Lp + j
                                                      (i < pair_L, j < pair_Lp, pair_Lp % 4 == 0, M == pair_L*pair_Lp): any residue
                                                      count L keeps 16-byte aligned pair rows inside the triangle multiplication
                                                      (split-f16 path only).  With C_split, c_split_L == pair_Lp */
    int a_pair;                                    /* A rows live in the UNpadded pair tensor: GEMM row (i,j) reads source row
                                                      i*pair_L + min(j, pair_L-1), or min(j, pair_L-1)*pair_L + i when
                                                      a_pair_transpose != 0 (k-contiguous fp32 A) */
    int c_pair;                                    /* C / gate / resid rows live in the UNpadded pair tensor: GEMM row (i,j) is
                                                      stored at row i*pair_L + j, rows with j >= pair_L are dropped (plain store) */
    /* Dual GEMM (split-f16 path, plain store): out = epi(A' B) * sigmoid(LN(A2) B2 + bias2) (+ resid) - the tail of the
     * TriangleMultiplication (seqformer.py:496-503: proj_out(final_norm(x)) * sigmoid(final_gate(norm(z)))) in one kernel.
     * A2: k-contiguous fp32 rows (K2 % 16 == 0), statistics inline; with pair_Lp > 0 its rows live in the UNpadded pair tensor. */
    const float* A2; long long sA2b, sA2m; int K2;
    const unsigned short* B2_split; long long sB23p, sB23n, sB23k;   /* gate weights as k-tiled planes (abx_split_weights_f16, b2_exp) */
    const float* ln2_csum; const float* bias2;     /* [N] column sums of the gamma-scaled gate weights, folded bias */
    /* Fused two-layer transition (split-f16 path, plain store; seqformer.py:358-376 LayerNorm -> Linear -> ReLU -> Linear + residual):
     * mlp != 0:  C = relu(LN(A) B + bias) B2 + bias2 (+ resid), the N-wide hidden activations never leave the CU.  A k-contiguous
     * fp32 with inline LayerNorm (ln_csum, ln_stats NULL), act = 1; N % 16 == 0 = hidden width; C / resid have N2 <= 192 columns;
     * B2_split = planes of the second layer's weights [N/16][2][N2][16] (strides sB23k / sB23p / sB23n) whose 16 k of every k-tile
     * are stored in the order 0-3, 8-11, 4-7, 12-15 (the accumulator layout of the first GEMM feeds the second one from
     * registers); C may alias resid and A (a block reads its rows before it writes them).
     * mlp = 2, the gated tail of the TriangleAttention (seqformer.py:300-312) in the same shape:
     *     C = (sigmoid(LN(A) B + bias) * gate) B2 + bias2 (+ resid)
     * act = 2; gate = the attention output [M][N] fp32 rows (sGm, sGb; 16-byte aligned), N = gate channels (N % 16 == 0); B2_split
     * in the permuted k order as above; C may alias resid and A. */
    int mlp, N2;
    /* LayerNorm over the N OUTPUT columns (gamma, beta; eps), applied right after bias / alpha / act and before rowscale / gate /
     * resid: Linear -> LayerNorm without a round trip of the rows through HBM (score_network.py:117-120).  Needs a kernel whose
     * wave tile holds whole rows: split-f16 path only (its own 128x128-tile instantiation), N <= 128, k-contiguous fp32 A, plain store */
    const float* out_ln_w; const float* out_ln_b; float out_ln_eps;
    int exact;                                     /* 0: large problems run on the float16 matrix cores from split operands
                                                      (3 exact products per fp32 product, fp32 accumulate - csrc/gemm3.hip);
                                                      1: always the exact fp32 MFMA kernel (v_mfma_f32_32x32x2_f32);
                                                      2: the split-f16 kernels whatever the problem size (falls back to the exact
                                                      kernel only on shape / alignment grounds): callers that need results
                                                      independent of the batch size fix the arithmetic per op with 1 or 2 */
    /* float16 weight planes: see "Split-f16 operands" above.  b_exp / b2_exp: exponents of B_split / B2_split (|.| <= 100) */
    int b_f16, b_exp, b2_exp;
    /* tune: 0 = library default.  A kernel-variant selector for A / B measurements and for the tests that cross-check two variants bit for
     * bit; every variant computes the same values.  Each kernel family reads its own bits only, so a value set for one family changes no
     * other launch.  Constants: ABX_TUNE_* below the struct.
     *   bit 0      NO_REMAP       workgroups keep the launch order (no XCD-contiguous remap, csrc/grid_map.h): gemm_kernel, gemm3_kernel
     *   bit 6      GTAIL_2WALK    gated attention tail: the two-walk form gemm3_gtail2w_kernel
     *   bit 7      DUAL_1WALK     dual GEMM, 96 < N <= 192: gemm3_dual1_kernel (one block per row tile, z walked once)
     *   bit 11     TILE_ONLY      the tile kernels of gemm3.hip for this call, never an A-stationary kernel of gemm_as.hip
     *   bits 12-13 ABLATE         gemm_as_kernel: 1 = no slice stores, 2 = no MFMA, 3 = half of the weight DMA (-DABX_AS_ABLATE builds only)
     *   bit 14     AS_DUAL        the dual descriptor of the TriangleMultiplication tail (A2, K = 128 channel-major, K2 = 192, N = 192, out
     *                             of place) takes gemm_as_dual_kernel also below its launch-size threshold of 1 024 blocks of 64 rows
     *                             (tests; the results are bit-identical to the tile kernel's either way)
     * Every other bit is refused (ABX_ERR_ARG, ABX_TUNE_LIVE_MASK): the variants they selected are retired, their measurements are in
     * DESIGN.md ("Retired GEMM variants").  Three retired fields keep their constant (FORCE 1-3, MLP_MINB1 4, NARROW_RING 9-10): their
     * kernels and dispatch lines are still compiled, unreachable behind the guard, for the reason given there.
     * Environment: ABX_NO_DUAL_AS set, not empty and not "0" keeps gemm3_dual_kernel for every dual descriptor of the process (A / B
     * measurements); the on / off switches all read that way.
     * The pair Transition (mlp = 1 with K = 192, N = 768, N2 = 192, a residual, plain fp32 rows in place or apart from the output, split-f16
     * route) takes gemm_as_mlp_kernel at ANY M - the choice is the shape class's, because that kernel sums the hidden channels in another
     * order than gemm3_mlp_kernel and a sample's bits must not depend on the launch; bit 11 keeps gemm3_mlp_kernel for the call,
     * ABX_NO_MLP_AS for the process */
    int tune;
    int c_planes_from, c_planes_group;             /* plain store, c_planes_from > 0: the output columns n >= c_planes_from leave as the B-side
                                                      OPERAND IMAGE of a following split-f16 product instead of fp32 - two float16 planes of
                                                      16 x value (p0 = f16(x'), p1 = f16(x' - p0): the same 4 bytes per element) in groups of
                                                      c_planes_group channels: channel n = c_planes_from + gi * G + ch of row m, plane p, sits at
                                                      byte  4 * (m * sCm + c_planes_from + gi * G) + p * 2 G + 2 ch  of C.  The k | v columns of
                                                      TriangleAttention's q | k | v projection (seqformer.py:520-531) are written this way
                                                      (from = 192, G = 48 = one head): the attention kernel stages them by DMA instead of loading,
                                                      splitting and writing them with a producer wave (AbxTriAttn.kv_planes).  from, G and N
                                                      multiples of 4, (N - from) % G == 0; no gate / glu / C_split / transposed store */
    int* range_flag; int range_tag;                /* range safety of the split-f16 kernels, optional DEVICE [1]: a workgroup whose accumulators
                                                      are not finite - what an operand beyond the split ranges above turns into, inf - inf,
                                                      and what a non-finite input gives too - ORs range_tag into *range_flag (one atomic per
                                                      wave, only then).  The caller clears the word, gives every call site its own bit, reads
                                                      it after a network call and repeats the call with exact = 1 (abx_amd/model/abx.py does) */
    unsigned long long* clock_probe;               /* diagnostics, optional DEVICE [2]: every workgroup of the split-f16 kernels adds
                                                      its elapsed shader-clock ticks (s_memtime) to [0] and its elapsed constant
                                                      100 MHz ticks (s_memrealtime) to [1]: 100 MHz * [0] / [1] = the shader clock
                                                      the kernel actually ran at (tools/probes/clock_probe.py) */
    int a_vec_ok, b_vec_ok, fast_ok;               /* filled by the library */
    int c_vec_ok, g_vec_ok, r_vec_ok, rs_vec_ok;   /* filled by the library (16-byte epilogue accesses possible) */
} AbxGemm;

/* AbxGemm.tune: the table at the field says what each selects */
#define ABX_TUNE_NO_REMAP 1
#define ABX_TUNE_GTAIL_2WALK 64
#define ABX_TUNE_DUAL_1WALK 128
#define ABX_TUNE_TILE_ONLY 2048
#define ABX_TUNE_ABLATE_SHIFT 12
#define ABX_TUNE_ABLATE_MASK (3 << ABX_TUNE_ABLATE_SHIFT)
#define ABX_TUNE_AS_DUAL 16384
/* retired and refused like every bit outside the mask below; named only by dispatch lines that stay compiled ("Retired GEMM variants") */
#define ABX_TUNE_FORCE_SHIFT 1
#define ABX_TUNE_FORCE_MASK (7 << ABX_TUNE_FORCE_SHIFT)
#define ABX_TUNE_MLP_MINB1 16
#define ABX_TUNE_NARROW_RING_SHIFT 9
#define ABX_TUNE_NARROW_RING_MASK (3 << ABX_TUNE_NARROW_RING_SHIFT)
/* the bits a descriptor may set: any other is refused where the descriptor is validated (launch and plan alike) */
#define ABX_TUNE_BITS_ (ABX_TUNE_NO_REMAP | ABX_TUNE_GTAIL_2WALK | ABX_TUNE_DUAL_1WALK | ABX_TUNE_TILE_ONLY | ABX_TUNE_AS_DUAL)
#ifdef ABX_AS_ABLATE
#define ABX_TUNE_LIVE_MASK (ABX_TUNE_BITS_ | ABX_TUNE_ABLATE_MASK)
#else
#define ABX_TUNE_LIVE_MASK ABX_TUNE_BITS_
#endif
int abx_gemm(const AbxGemm* desc, hipStream_t stream);
/* Two GEMMs over the SAME rows in one launch: `main_gemm` a plain-store split-f16 problem with N % 128 == 0 (k-contiguous fp32 A), `side_gemm` a
 * skinny (N <= 32) transposed-store projection - TriangleAttention's q | k | v | gate projection and its pair bias, which both read
 * LayerNorm(z) (seqformer.py:520-531).  The side tiles are dealt between the main tiles of the grid, so the skinny projection reads its
 * A panel from the L2 the main tiles have just filled instead of streaming the 9.5 GB pair tensor from HBM in a launch of its own.
 * Bit-identical to abx_gemm(main_gemm) + abx_gemm(side_gemm), which is also what it does when the pair does not qualify. */
int abx_gemm_side(const AbxGemm* main_gemm, const AbxGemm* side_gemm, hipStream_t stream);
/* 1 when an abx_gemm_side launch over M rows takes the kernel that can write plane output (AbxGemm.c_planes_from), else 0 */
int abx_gemm_planes_ok(long long M);
/* the mode table above, without a launch: 0 or a negative code (abx_last_error_string names the offending pair / requirement) */
int abx_gemm_check_modes(const AbxGemm* desc);
/* fp32 weights W[n][k] -> out[Kp/16][2][N][16] float16 planes (p0, p1) of w * 2^scale_exp (see AbxGemm.b_f16); the caller picks
 * scale_exp = 14 - e with max|w| = m * 2^e, 0.5 <= m < 1 (so that max|w| * 2^scale_exp is in [2^13, 2^14)) */
int abx_split_weights_f16(const float* w, long long s_n, long long s_k, int N, int K, int scale_exp, unsigned short* out, hipStream_t stream);
/* The tail of an IPA layer on the single representation s (M = B*L rows of C = 256 channels), reference score_network.py:126-163 /
 * folding.py (per layer, after the attention): s <- LN1(s + feat W_final + b_final); s <- LN2(s + relu(relu(s W0 + b0) W2 + b2) W4 + b4)
 * (attention_module.final_proj + attention_layer_norm + transition_module.0/.2/.4 + transition_layer_norm) in ONE launch: the
 * intermediate activations never leave the CU (split-f16 arithmetic of AbxGemm; weights as abx_split_weights_f16 planes
 * [K/16][2][256][16] with their exponents).  s is updated in place. */
typedef struct AbxIpaTail {
    const float* feat; long long s_feat;           /* IPA features (M, K1), row stride in floats (K1 % 16 == 0) */
    float* s; long long s_s;                       /* (M, 256) in / out */
    int M, K1, C;                                  /* C must be 256 */
    const unsigned short* W_final; int e_final; const float* b_final;
    const float* ln1_w; const float* ln1_b;
    const unsigned short* W_t0; int e_t0; const float* b_t0;
    const unsigned short* W_t2; int e_t2; const float* b_t2;
    const unsigned short* W_t4; int e_t4; const float* b_t4;
    const float* ln2_w; const float* ln2_b;
    float ln_eps;
    /* optional (W_aff != NULL): affine_update (W_aff [256][6] fp32, b_aff [6]) of the new s and the frame update of abx_rigid_update
     * (same operands: fixed_mask, init / current frames, accumulated quaternion, position scale) in the same launch */
    const float* W_aff; const float* b_aff;
    const int* fixed; const float* init_q; const float* init_t;
    float* cur_q; float* cur_t; float* cur_R; float* delta_q; float pscale;
    int* range_flag; int range_tag;                /* see AbxGemm.range_flag: set when the layer's output rows are not finite */
    /* optional (partial != NULL): feat W_final arrives as n_partial K-slice products (each (M, 256) fp32, s_partial floats apart) of a
     * split-K abx_gemm launched before (batch = slice: sAb = K1 / n_partial, sB3b = (K1 / n_partial / 16) * sB3k, sCb = s_partial); the kernel adds
     * them in slice order instead of walking K1 itself - a 32-row block's 132-k-step DMA chain at K1 = 2 112 is what a layer costs at
     * small batches.  feat / W_final / K1 are then unused. */
    const float* partial; int n_partial; long long s_partial;
} AbxIpaTail;
int abx_ipa_tail(const AbxIpaTail* desc, hipStream_t stream);
/* The per-residue heads on the final single representation in ONE launch (split-f16 arithmetic of AbxGemm, activations resident on the
 * CU): TorsionModule (abx/model/sidechain.py:28-62: proj_act + proj_init_act, two ResNet blocks, projection -> 14 unnormalised
 * sin / cos), SequenceHead.net (abx/model/head.py:143-163: LayerNorm, 256 -> 128 -> 128 -> 20) and, when W_p1 != NULL,
 * PredictedLDDTHead.net (head.py:206-226: LayerNorm, 256 -> 128 -> 128 -> 50).  Weights as abx_split_weights_f16 planes
 * [K/16][2][128][16] of the (K, 128) transposed weight with their exponents; the 14 / 20 / 50-column projections ZERO-PADDED to 128
 * columns (planes and [128] biases).  Thirteen (eighteen) abx_gemm / abx_layernorm calls otherwise. */
typedef struct AbxHeadsTail {
    const float* s; long long s_s;                 /* (M, 256) structure-module output, row stride in floats */
    const float* s0; long long s_s0;               /* (M, 256) initial single representation (init_seq_layer_norm output) */
    int M;
    const unsigned short* W_act; int e_act; const float* b_act;        /* torsion_module.proj_act.1       256 -> 128 */
    const unsigned short* W_init; int e_init; const float* b_init;     /* torsion_module.proj_init_act.1  256 -> 128 */
    const unsigned short* W_r0; int e_r0; const float* b_r0;           /* blocks.0.net.1 */
    const unsigned short* W_r1; int e_r1; const float* b_r1;           /* blocks.0.net.3 */
    const unsigned short* W_r2; int e_r2; const float* b_r2;           /* blocks.1.net.1 */
    const unsigned short* W_r3; int e_r3; const float* b_r3;           /* blocks.1.net.3 */
    const unsigned short* W_proj; int e_proj; const float* b_proj;     /* projection 128 -> 14 (padded) */
    float* un;                                                         /* (M, 14) out */
    const float* lns_w; const float* lns_b;                            /* sequence_module.net.0 (LayerNorm [256]) */
    const unsigned short* W_s1; int e_s1; const float* b_s1;           /* net.1 256 -> 128 */
    const unsigned short* W_s3; int e_s3; const float* b_s3;           /* net.3 128 -> 128 */
    const unsigned short* W_s5; int e_s5; const float* b_s5;           /* net.5 128 -> 20 (padded) */
    float* logits;                                                     /* (M, 20) out */
    const float* lnp_w; const float* lnp_b;                            /* predicted_lddt.net.0; the head is optional (W_p1 == NULL: skipped) */
    const unsigned short* W_p1; int e_p1; const float* b_p1;
    const unsigned short* W_p3; int e_p3; const float* b_p3;
    const unsigned short* W_p5; int e_p5; const float* b_p5;           /* 128 -> 50 (padded) */
    float* pl;                                                         /* (M, 50) out */
    float ln_eps;
    int* range_flag; int range_tag;                /* see AbxGemm.range_flag: set when an output value is not finite */
} AbxHeadsTail;
int abx_heads_tail(const AbxHeadsTail* desc, hipStream_t stream);
/* diagnostics: resident workgroups per CU of the main split-f16 GEMM instantiations (0: 128x192, 1: 128x128,
 * 2: 128x128 transposed store, 3: 128x192 plane operands); negative on error */
int abx_gemm3_occupancy(int which);
/* diagnostics: the name of the kernel instantiation abx_gemm(main_gemm) (side_gemm == NULL) or abx_gemm_side(main_gemm, side_gemm) would
 * launch, as `rocprofv3 --stats` spells it ("gemm3_kernel<128, 128, 32, 128, 0, false, 4>"), written to name[cap].  The dispatch itself
 * runs, up to the launch: the same validation (a rejected descriptor returns the same negative code), the same environment switches and
 * tune bits; a pair that falls back to two launches gives the main launch's name.  No HIP runtime call and no operand is dereferenced:
 * works without a GPU, on placeholder addresses (their alignment and overlap are looked at). */
int abx_gemm_plan(const AbxGemm* main_gemm, const AbxGemm* side_gemm, char* name, int cap);

/* LayerNorm statistics (mean, rstd) per row for the LN-on-load GEMM prologue (torch.nn.LayerNorm, eps 1e-5).
 * s_k == 1: rows dense over batch (row stride s_row); else channel-major: element (b,row,k) at x + b*s_b + k*s_k + row. */
int abx_row_stats(const float* x, long long s_b, long long s_row, long long s_k, int batch, int rows, int K, float eps,
                  float* stats, hipStream_t stream);
/* materialised LayerNorm over contiguous rows, out = (res?) + LN(x)  (seqformer.py:216-221 prev_*_norm, score_network.py:119-133) */
int abx_layernorm(const float* x, long long s_row, long long rows, int K, const float* gamma, const float* beta, float eps,
                  float* out, long long s_out, const float* res, long long s_res, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Attention kernels
 * ---------------------------------------------------------------------------------------------------------- */
/* Flash-style triangle attention (seqformer.py:506-550 + Attention.forward split_first=True :272-312):
 * per (b, row s, head h): softmax_k( q.k * scale + bias[b,h,q,k] + keymask ) v, then * sigmoid(gate).
 * q,k,v,gate: element (b,s,l,h,d) at ptr + b*sb + s*ss + l*sl + h*D + d.  per_column orientation = swapped ss/sl. */
typedef struct AbxTriAttn {
    const float* q; const float* k; const float* v; const float* gate;
    long long sb, ss, sl;
    const float* bias; long long bias_sb, bias_sh, bias_sq, bias_sk;
    const float* keymask; long long km_sb;          /* float 0/1 [b*km_sb + k] or NULL */
    float* out; long long ob, os, ol;               /* out (b,s,l,h*D+d) */
    int B, S, L, H, D;                              /* D must be 48 */
    float scale;
    int exact;                                      /* 0: split-f16 matrix-core kernel (csrc/attention.hip tri_attn8_kernel; any L): keys / values
                                                       staged as two float16 planes of 16 x (|k|, |v| < 4095; 2^-29 absolute below 2^-6),
                                                       queries as two pieces of q * scale * log2(e) * 8 (|q * scale| < 5600), softmax weights
                                                       as two pieces of P * 2^8: 3 exact float16 products per fp32 product, fp32 accumulate;
                                                       an operand beyond its range gives NaN in its output rows, never a wrong number;
                                                       1: exact fp32 MFMA kernel (v_mfma_f32_16x16x4_f32; keys in chunks: any L) */
    unsigned long long* clock_probe;                /* diagnostics, optional DEVICE [2] (see AbxGemm.clock_probe; split-f16 kernels) */
    int* range_flag; int range_tag;                 /* see AbxGemm.range_flag: set when a query row's output is not finite (split-f16 kernels) */
    int tune;                                       /* 0 = library default (persistent workgroups, two query tiles per wave walked together);
                                                       bit 1: the other key-chunk size (128 <-> 192; bit-identical results); bit 2: the round-3
                                                       kernel tri_attn4 (one workgroup per row, one query tile at a time; with bit 0: without
                                                       its producer wave) - benchmarking and cross-checks: its accumulation order differs */
    int bias_log2;                                  /* 1: `bias` holds ABX_TRI_BIAS_LOG2 x the pair bias - the projection that wrote it applied the
                                                       factor (AbxGemm.alpha), so the split-f16 kernel adds it to its accumulators as it is: the
                                                       same bits as the multiplication in the kernel (one rounding of the same product), 32 vector
                                                       instructions less per pair of query tiles and key tile.  abx_tri_attn_block_fwd does this. */
    int kv_planes;                                  /* 1: k and v do not point to fp32 rows but to the operand images AbxGemm.c_planes_from writes: per
                                                       key and head [plane p0: 48 float16 | plane p1: 48 float16] of 16 x value at the byte address
                                                       the fp32 head slice would have (192 bytes either way: same pointers, same strides).  Split-f16
                                                       kernel tri_attn8 only (exact = 0, tune = 0): its producer wave turns into a DMA issuer
                                                       (global_load_lds straight into the chunk buffers: no registers, no split, no LDS writes) */
    int q_parts, row_groups;                        /* filled by the library */
} AbxTriAttn;
/* float(log2 e) * 2^7: base-2 logits in the accumulator units of tri_attn8_kernel */
#define ABX_TRI_BIAS_LOG2 (1.4426950408889634f * 128.0f)
int abx_tri_attn_fwd(const AbxTriAttn* desc, hipStream_t stream);

/* Triangle attention with the q | k | v projection of the row inside (csrc/attention.hip tri_attn8_rowfused_kernel): replaces the
 * LayerNorm -> proj_q | proj_k | proj_v GEMM (seqformer.py:520-529, :527-548) AND abx_tri_attn_fwd (Attention.forward :272-312) for rows of
 * L <= ABX_TRI_ROWFUSED_LMAX.  q, k, v of pair row (b, s) are computed from z[b, s, :, :] in the workgroup that attends over that row (the
 * arithmetic of the split-f16 GEMM: same pieces, same products in the same order, same folded-LayerNorm epilogue) and never reach memory;
 * the output is bit-identical to abx_gemm (exact = 2, LayerNorm folded) followed by abx_tri_attn_fwd (exact = 0, bias_log2 as given).
 * AbxTriRowPack: the q | k | v pack re-ordered per head ([k 48 | v 48 | q 48 + 16], columns permuted to the kernel's fragment order) by
 * abx_tri_rowpack into caller memory of abx_tri_rowpack_bytes() (256-byte aligned; set-up work, asynchronous on the stream). */
typedef struct AbxTriRowPack {
    const unsigned short* planes;       /* [H][15 stages][4 k-tiles][2 planes][32 columns][16] float16 */
    const float* csum;                  /* [H][160] column sums (folded LayerNorm) in packed column order */
    const float* bias;                  /* [H][160] */
    int b_exp;                          /* exponent of the planes (that of the source pack) */
    int H;                              /* heads: 4 */
} AbxTriRowPack;
#define ABX_TRI_ROWFUSED_LMAX 352
long long abx_tri_rowpack_bytes(void);
/* (abx_tri_rowpack: declared with AbxLinearPack below) */
/* 1 when abx_tri_attn_block_fwd takes the row-fused route for rows of length L: L <= ABX_TRI_ROWFUSED_LMAX (a function of L alone, never of
 * the batch: a sample's bits do not depend on how many samples share a launch) and the environment variable ABX_NO_TRI_ROWFUSED is not
 * set to something other than "0" (A/B measurements: forces the two launches). */
int abx_tri_attn_rowfused_ok(int L);
/* desc: as for abx_tri_attn_fwd with exact = 0, gate = NULL, kv_planes = 0, q_parts unused; q / k / v / sb / ss / sl are ignored; keymask
 * may be NULL (no key masked).  The bias must be
 * key-contiguous rows padded to a multiple of 4 floats, 16-byte aligned (bias_sk == 1: what abx_tri_attn_block_fwd passes).
 * z: the pair rows, element (b, s, l, c) at z + b*zb + s*zs + l*zl + c (192 channels; the orientation is in zs / zl like ss / sl).
 * slot_order: 0 = (b, row, h): the four heads of a row run on neighbouring workgroups of one XCD (z[b, s] is fetched from HBM once);
 * 1 = (b, h, row): the order of tri_attn8_kernel (one bias map per XCD, z fetched four times); -1 = library default. */
int abx_tri_attn_rowfused_fwd(const AbxTriAttn* desc, const float* z, long long zb, long long zs, long long zl, const AbxTriRowPack* pack,
                              int slot_order, hipStream_t stream);
/* How the kernel's issuing wave warms the L2 with the z rows (TriRowArgs.touch, csrc/tri_row_touch.h): 0 = not at all, 1 = the whole
 * next row at the start of the attention phase, 2 = per k-group just ahead of the projection's walk.  Same bits for all three; the
 * default is 0 (the one that measures fastest on the whole step).  The start value comes from the environment variable ABX_TRI_ROW_TOUCH (0 | 1 | 2, read once, on the C side only: A / B
 * measurements).  v = 0, 1, 2: the setting of later launches of this process; any other v changes nothing.  Returns the setting that held
 * before the call. */
int abx_tri_row_touch(int v);
/* diagnostics: the name of the kernel abx_tri_attn_fwd(desc) (rowfused == 0) or abx_tri_attn_rowfused_fwd(desc, z rows with the strides
 * desc->sb / ss / sl, ...) (rowfused != 0) would launch, written to name[cap]; the descriptor is validated as by the entry point and a
 * rejected one returns the same negative code.  No HIP runtime call, no operand dereferenced: works without a GPU (see abx_gemm_plan). */
int abx_tri_attn_plan(const AbxTriAttn* desc, int rowfused, char* name, int cap);

/* Sequence attention with pair bias (seqformer.py:314-356 + Attention.forward split_first=False :278-312).
 * qkv: [B*L][H*3*D] with per-head layout [q D | k D | v D]; bias [b][h][q][k]; gate pre-activation [B*L][H*D];
 * out [B*L][H*D] = softmax(...) v * sigmoid(gate).  D <= 32. */
int abx_seq_attn_fwd(const float* qkv, const float* bias, const float* keymask, const float* gate, float* out, int B, int L,
                     int H, int D, float scale, hipStream_t stream);
/* diagnostics: the name of the kernel instantiation abx_seq_attn_fwd launches for one sample of length L (32 heads of 17 channels), written
 * to name[cap], and - qblk not null - the query rows per workgroup of that launch (the grid's x extent is ceil(L / *qblk)).  A length the
 * entry point refuses returns the same negative code and message.  No HIP runtime call, no operand dereferenced (see abx_gemm_plan). */
int abx_seq_attn_plan(int L, char* name, int cap, int* qblk);

/* Invariant Point Attention core (folding.py:47-132).  abx_ipa_pack turns the fused projection rows
 * [q_scalar 192 | kv_scalar 384 | q_point_local 144 | kv_point_local 432] into global-frame packs
 * (r3.rigids_apply, r3.py:9-16); abx_ipa_attn does logits (scalar + point distance + pair bias), mask, softmax_j and the
 * three outputs (scalar, points back in the local frame + norms, attention over the pair slab), writing the
 * 2112-wide concat [scalar | points (r n) | norms | pair] that final_proj consumes.  Two launches: the attention weights
 * (kept in attn_ws [B][L][3 head groups][L][4] fp32, abx_ipa_attn_workspace_bytes) with the scalar / point outputs, then the stream over
 * the pair slab z [B][L][L][128]. */
int abx_ipa_pack(const float* proj, const float* rots, const float* trans, float* qpack, float* kpack, float* vpack,
                 int B, int L, float scalar_weight, hipStream_t stream);
int abx_ipa_attn(const float* qpack, const float* kpack, const float* vpack, const float* bias2d, const float* z,
                 const float* mask, const float* rots, const float* trans, const float* point_weights /* [12] */,
                 float* attn_ws, float* feat, int B, int L, hipStream_t stream);
/* the two launches of abx_ipa_attn, separately callable (profiling; feat rows: weights writes [0, 576), pair writes [576, 2112)) */
int abx_ipa_weights(const float* qpack, const float* kpack, const float* vpack, const float* bias2d, const float* mask,
                    const float* rots, const float* trans, const float* point_weights, float* attn_ws, float* feat, int B, int L,
                    hipStream_t stream);
int abx_ipa_pair(const float* attn_ws, const float* z, float* feat, int B, int L, hipStream_t stream);
long long abx_ipa_attn_workspace_bytes(int B, int L);
long long abx_ipa_qpack_bytes(int B, int L);   /* size of qpack: query rows padded to blocks of 12, pairs interleaved */

/* ------------------------------------------------------------------------------------------------------------
 * Embedding assembly (seqformer.py:49-119,170-223) and small pair-stack helpers
 * ---------------------------------------------------------------------------------------------------------- */
/* sinusoidal embedding of t*10000 (double product, then float) -> [B][dim]; freqs [dim/2] = exp(arange * -ln(1e4)/(dim/2-1)) */
int abx_timestep_embedding(const double* t, const float* freqs, int B, int dim, float* out, hipStream_t stream);
/* seq_act[b,l] = [ seq_static[b,l] (+ aa_table[seq_t[b,l]] for l < Lab) | temb[b] ] + LN(prev_seq[b,l]) */
int abx_assemble_seq(const float* seq_static, long long ss_b, const float* aa_table, const long long* seq_t, int Lab,
                     const float* temb, const float* prev_seq, const float* gamma, const float* beta, float* out, int B,
                     int L, int C, int E, hipStream_t stream);
/* pair_act[b,i,j] = [ pair_static[b,i,j] | temb[b] | temb[b] ] + LN(prev_pair[b,i,j]) + pos_table[prev_pos[b,i,j]];
 * stats_out (optional): LayerNorm (mean, rstd) of every assembled row for the first consumer */
int abx_assemble_pair(const float* pair_static, long long ps_b, const float* temb, const float* prev_pair,
                      const float* gamma, const float* beta, const long long* prev_pos, const float* pos_table, float* out,
                      float* stats_out, int B, int L, int C, int E, hipStream_t stream);
/* Pair-representation assembly AND the sequence attention's pair bias in one pass over the pair rows (round 6; seqformer.py:193-223 + :324-333):
 * out = z0 as abx_assemble_pair writes it (C = 128, E = 32: 192 channels) and biasT[b][h][i*L + j] = Linear(LayerNorm(z0[b,i,j,:]))[h] for 32 heads -
 * what abx_gemm computes from z0 with a folded LayerNorm (w_planes = abx_split_weights_f16 planes [12][2][32][16] of the gamma-scaled weight with
 * exponent w_exp, csum its column sums, bias the folded bias; split-f16 arithmetic, range_tag as AbxGemm.range_flag).  One workgroup per (b, i)
 * row of the pair tensor; the 9.5 GB second read of z0 by a projection launch of its own is gone. */
int abx_assemble_pair_bias(const float* pair_static, long long ps_b, const float* temb, const float* prev_pair, const float* gamma,
                           const float* beta, const long long* prev_pos, const float* pos_table, float* out, const unsigned short* w_planes,
                           int w_exp, const float* csum, const float* bias, float ln_eps, float* biasT, int B, int L, int* range_flag,
                           int range_tag, hipStream_t stream);
/* OuterProductMean features (seqformer.py:400-409): feat[b,i,j] = [ left[b,j]*right[b,i] | left[b,j]-right[b,i] ];
 * left/right rows have stride ld floats */
int abx_opm_features(const float* left, const float* right, long long ld, float* feat, int B, int L, int C,
                     hipStream_t stream);
/* OuterProductMean without its feature tensor (seqformer.py:395-411; round 6): z[b,i,j,:] += out_proj([l_j * r_i | l_j - r_i]) evaluated as
 * l_j . (diag(r_i) W1 + W2) + (bias - r_i . W2) - one workgroup per (b, i) row of the pair tensor builds the 64 x 192 operand image of its row
 * in LDS and streams the L positions j; HBM traffic = z read + z written (the (B, L, L, 128) feature tensor of abx_opm_features + the K = 128
 * abx_gemm over it: 31.7 GB per call at 100 samples of L = 352 instead of 19 GB).  lr: [B*L][ld] rows [left 64 | right 64] (already masked),
 * Wt: out_proj.weight^T [128][192] fp32 (rows 0..63 against the products, 64..127 against the differences), bias [192] or NULL, z updated
 * in place.  Split-f16 arithmetic (3 exact products per fp32 product, fp32 accumulate; |diag(r) W1 + W2| < 4095, else NaN and range_tag is
 * OR-ed into *range_flag - see AbxGemm.range_flag; the caller's exact route is abx_opm_features + abx_gemm with exact = 1). */
int abx_opm_out_fwd(const float* lr, long long ld, const float* Wt, const float* bias, float* z, int B, int L, int* range_flag, int range_tag,
                    hipStream_t stream);
/* out[n][a][b] = in[n][b][a] (transpose != 0) or in[n][a][b] for nmat L x L matrices, output rows padded to Lp >= L floats (pad
 * columns = 0).  The triangle attention reads its (4, L, L) pair bias key-contiguously in rows of Lp % 4 == 0 floats (16-byte
 * loads for any residue count); the ending-node orientation reads it transposed ('b i j c -> b j i c', seqformer.py:536) */
int abx_transpose_last2(const float* in, float* out, int nmat, int L, int Lp, int transpose, hipStream_t stream);
/* pair mask[b,i,j] = mask[b,i]*mask[b,j], rows of Lp >= L entries (columns j >= L are written as 0: the padded pair rows of
 * AbxGemm.pair_Lp) */
int abx_pair_mask(const float* mask, float* out, int B, int L, int Lp, hipStream_t stream);

/* Trajectory-invariant encoders (encoder.py:123-269, seqformer.py:177-206): gather/concat stages; the MLPs run on abx_gemm. */
int abx_pair_embed_features(const long long* aa, const int* chain_id, const int* residx, const float* atom14,
                            const unsigned char* atom14_exists, const float* aa_pair_embed, const float* relpos_embed,
                            const float* distcoef, const float* dgram_embed, const float* sq_breaks /* [14] */,
                            float* feat512, float* dist196, int B, int L, hipStream_t stream);
int abx_relpos_block(const int* residx, const float* table, float* out, int B, int L, int Lab, int C, int max_rel,
                     hipStream_t stream);
int abx_gather_rows(const float* table, const long long* idx, const float* rowscale, float* out, long long s_out, long long n,
                    int C, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Rigid frames, torsions, heads (score_network.py:100-194, quat_affine.py, r3.py, atom.py, sidechain.py:64-90, head.py:162-226)
 * ---------------------------------------------------------------------------------------------------------- */
/* rigids_t (B,L,7) f32 or f64 -> init_q, init_t (unscaled), cur_q, cur_t (= init_t/position_scale), cur_R, delta_q = identity */
int abx_frames_init(const void* rigids_t, int is_f64, float* init_q, float* init_t, float* cur_q, float* cur_t, float* cur_R,
                    float* delta_q, int n, float position_scale, hipStream_t stream);
/* one IPA layer tail: quat_precompose_vec on delta and current, translation update with the OLD rotation, fixed-mask restore,
 * quat_to_rot (score_network.py:137-149) */
int abx_rigid_update(const float* upd6, const int* fixed_mask, const float* init_q, const float* init_t, float* cur_q,
                     float* cur_t, float* cur_R, float* delta_q, int n, float position_scale, hipStream_t stream);
/* final quaternion, igso3 rot score (cached table lookup, so3_diffuser.py:264-297), r3 trans score (r3_diffuser.py:158-164),
 * rigids (B,L,7).  t is (B,) double; t_is_f32 selects the reference's fp32 arithmetic of the warm-up call.
 * trans_score is written as double when !t_is_f32 else float. */
typedef struct AbxScoreArgs {
    const float* init_q; const float* init_t; const float* delta_q; const float* cur_t; const int* fixed_mask;
    const double* t; int t_is_f32;
    const float* score_norms; int num_sigma, num_omega; const float* discrete_sigma; const float* discrete_omega;
    float exp_max_sigma, exp_min_sigma;     /* fp32 exp(1.5), exp(0.1) as torch computes them */
    float min_b, bdiff;                     /* fp32 0.1, 19.9 */
    float coord_scale;                      /* fp32 0.1 */
    float position_scale;
    float* rot_score; void* trans_score; float* rigids;
    int B, L;
} AbxScoreArgs;
int abx_scores(const AbxScoreArgs* a, hipStream_t stream);
/* torsion head tail: l2-normalise (eps 1e-12) and take ground-truth torsions at fixed residues (sidechain.py:67-72) */
int abx_torsion_finalize(const float* unnorm, const float* gt_sincos, const int* fixed_mask, float* angles, int n,
                         hipStream_t stream);
/* SequenceHead tail (head.py:165-199): seq_0 = argmax(logits) merged with seq_t at fixed positions; frames from torsions;
 * atom14 and atom37 with the seq_0 residue tables. tables: default_frames (21,8,4,4), group_idx (21,14) int, lit_pos (21,14,3) */
int abx_seq_head_atoms(const float* logits, const int* fixed_mask, const long long* seq_t, const float* rigids,
                       const float* angles, const long long* atom37_to_atom14, const float* default_frames,
                       const int* group_idx, const float* lit_pos, long long* seq_0, float* atom14, float* atom37, int n,
                       hipStream_t stream);
/* The same under a sequence-constraint table (NOT in the reference: head.py:166-167 takes the plain maximum): seq_bias DEVICE float32
 * (L,20), row i % L for residue i of the n = B * L, a finite logit bias or -inf (forbidden letter).  seq_0 = argmax(logits + seq_bias),
 * first maximum wins, merged with seq_t at fixed positions; frames and atoms are built from that residue type by the same kernel body.
 * The logits buffer is read only: the caller's logits stay the network's own. */
int abx_seq_head_atoms_biased(const float* logits, const int* fixed_mask, const long long* seq_t, const float* rigids,
                              const float* angles, const long long* atom37_to_atom14, const float* default_frames,
                              const int* group_idx, const float* lit_pos, long long* seq_0, float* atom14, float* atom37, int n,
                              const float* seq_bias, int L, hipStream_t stream);
/* get_prev (abx.py:17-26): virtual C-beta from N,CA,C (common_modules.py:62-83) and 15-bin distogram -> int64 (B,L,L) */
int abx_prev_pos(const float* atom37, const float* sq_breaks, int num_breaks, long long* prev_pos, int B, int L,
                 hipStream_t stream);
/* pLDDT = 100 * sum softmax(logits) * bin centres (utils.py:158-171) */
int abx_plddt(const float* logits, float* out, int n, int bins, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Diffuser (diffuser/so3_diffuser.py, r3_diffuser.py, discrete_diffuser.py, full_diffuser.py:174-227)
 * ---------------------------------------------------------------------------------------------------------- */
/* IGSO(3) series tables (so3_diffuser.py:15-49,72-112,153-166): pdf, cdf, score_norms [num_sigma][num_omega] */
int abx_igso3_tables(const float* sigma, const float* omega, int num_sigma, int num_omega, int L_terms, float* pdf, float* cdf,
                     float* score_norms, hipStream_t stream);
/* One reverse step of all three processes in float64 with injected or device-generated noise, mask merge after all three.
 * rigid_in f32 or f64 (B,L,7); rot_score f32; trans_score f64 (or f32 when ts_is_f32); logits f32 (B,L,20); t (B,) double.
 * Noise: z_rot,z_trans f32 (B,L,3), jumps f32 (B,L,20) when given; otherwise Philox4x32-10 keyed by (seed, sample id, residue, step).
 * The Poisson jump counts (discrete_diffuser.py:182-183) are a pure function of one uniform each: the inverse cdf of
 * Poisson(rate*dt) (fp32 pmf recurrence from (float)exp(-(double)lam), see diffuser.hip::poisson_icdf) evaluated at
 * u_jumps[b,l,s] in (0,1) when given (jumps == NULL), else at the Philox uniform of (sample id, residue, step, draw s).
 * Outputs rigid_out f64 (B,L,7), seq_out int64 (B,L).  Optional: rates_out (B,L,20) = the Poisson rates * dt,
 * jumps_out (B,L,20) = the jump counts that were applied.
 * Sequence constraints (NOT in the reference: discrete_diffuser.py:150-188 has no such handle): seq_bias, optional DEVICE float32
 * (L,20) shared by all samples, row l = residue l: a finite logit bias (0: no opinion) or -inf (the letter is forbidden there).  With
 * it the softmax of discrete_diffuser.py:160 runs over logits + seq_bias, the Poisson rate of a forbidden target is exactly 0 (as it is
 * for the current token; rates_out / jumps_out report the zeros), one uniform is consumed per target all the same, and a leap whose
 * ordinal landing token clamp(x_t + sum jumps * (s - x_t)) (discrete_diffuser.py:184-188) is forbidden is rejected: the token stays.
 * A forbidden x_t leaves with the first leap that lands on an allowed letter; a row without a finite entry keeps its token.  The
 * caller keeps rows of residues outside diffuse_mask at 0 and refuses +inf / NaN.  seq_bias == NULL is the reference's step. */
typedef struct AbxReverseArgs {
    const void* rigid_in; int rigid_is_f64;
    const long long* seq_in;
    const float* rot_score; const void* trans_score; int ts_is_f32; const float* logits;
    const int* diffuse_mask; const double* t; float dt;
    const float* z_rot; const float* z_trans; const float* jumps;
    const float* u_jumps;                    /* optional (B,L,20) uniforms in (0,1) driving the Poisson inverse cdf (jumps == NULL) */
    const float* dt_dev;                     /* optional DEVICE float: overrides `dt` (the reference's loop passes dt as a 0-dim
                                                device tensor, inference.py:198-199: no device-to-host read on the step path) */
    unsigned long long seed; const long long* sample_ids; int step;
    const int* step_dev;                     /* optional DEVICE int: overrides `step` (a hipGraph-captured reverse step reads the
                                                current step index at replay time instead of a value frozen at capture) */
    float exp_max_sigma, exp_min_sigma, min_b, bdiff, coord_scale, rate_const;
    float noise_scale; int center;
    double* rigid_out; long long* seq_out; float* rates_out; float* jumps_out;
    int B, L;
    const float* seq_bias;                   /* optional DEVICE (L,20): logit bias / -inf = forbidden letter per residue (see above) */
} AbxReverseArgs;
int abx_reverse_step(const AbxReverseArgs* a, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Guidance terms (north_star "guidance pairwise-distance / clash terms").  NOT in the reference's sampler
 * (its loop runs under no_grad): an opt-in extension built from the violation material the reference ships -
 * van-der-Waals radii / overlap tolerance (abx/common/residue_constants.py:381-386,483-525, config/config_model.json:116,213-214)
 * and the C-N peptide-bond term of eval/metric_scripts/cal_vio.py:29-74.  Per sample:
 *   energy[b] = { w_clash * sum_pairs w_ij relu(r_a + r_b - overlap_tolerance - d_ab),
 *                 w_bond  * sum_i relu(|d(C_i,N_i+1) - l0| - tol * sigma),
 *                 w_angle * sum_i [ relu(|cos(CA_i,C_i,N_i+1) - c1| - tol * s1) + relu(|cos(C_i,N_i+1,CA_i+1) - c2| - tol * s2) ] }
 *   (|.| smoothed as sqrt(1e-6 + .^2); l0 / sigma proline-aware; c1 = -0.4473 +- 0.0311, c2 = -0.5203 +- 0.0353: cal_vio.py:76-105,
 *   abx/common/residue_constants.py:475-480)
 *   grad_atom = dE/dx (B,L,14,3);  grad_trans = sum_a g_a;  grad_rot = sum_a (x_a - frame_trans) x g_a   (B,L,3) each.
 * Pairs of one residue, the peptide bond C(i)-N(i+1) of linked neighbours and SG-SG pairs are excluded from the clash term; w_ij =
 * between_chain_factor for atoms of different chains.  Residues i, i+1 are linked when they share a chain id and, if residx is
 * given, residx[i+1] == residx[i] + 1 (residx == NULL: the chain-only rule of cal_vio.py:51).
 * radius: [21][14] van-der-Waals radius of every atom14 slot (0 for empty slots).
 * The caller allocates the workspace (abx_clash_grad_workspace_bytes). */
typedef struct AbxGuidanceArgs {
    const float* atom14; const unsigned char* atom_mask; const long long* aatype; const int* chain_id;
    const int* residx;                              /* optional residue numbers (B,L) */
    const float* radius; const float* frame_trans;
    float overlap_tolerance, between_chain_factor, bond_tolerance_factor, w_clash, w_bond, w_angle;
    float* energy;                                  /* (B,3): clash, bond, angle */
    float* grad_atom; float* grad_trans; float* grad_rot;
    int B, L;
} AbxGuidanceArgs;
long long abx_clash_grad_workspace_bytes(int B, int L);
int abx_clash_grad(const AbxGuidanceArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Interface guidance terms (north_star "the evolutionary/physical/geometric guidance-gradient terms" and "guidance pairwise-distance
 * / clash terms": the geometric half, beside the physical half of abx_clash_grad).  An EXTENSION WITH NO REFERENCE SITE: the reference
 * samples without guidance.  Reference constants used: the 4 A heavy-atom contact distance of the interface table
 * (abx_interface_scores `cutoff`, n_contact_region), the 8 A pseudo-beta contact distance of upstream's MetricDictHead
 * (abx_distogram_scores `contact_cutoff`) and the pseudo-beta rule (CB, slot 4, else CA, slot 1) of its distogram features.
 * The caller hands ONE structure per sample: atom14 / atom_mask already hold, per row, the predicted atoms where moved[b, r] is set
 * and the ground truth elsewhere.  d = sqrt(1e-10 + |x_a - x_b|^2) everywhere (as in abx_clash_grad).  Per sample:
 *   energy[b][0] = -w_contact * sum s(d_ab),  a: existing atoms of moved rows, b: existing atoms of rows with target[r] set that are
 *                  not moved;  s = 1 (d <= d0), (1 - u^2)^2 with u = (d - d0) / (d1 - d0) (d0 < d < d1), 0 (d >= d1)
 *   energy[b][1] = w_hot * sum_h Hub(m_h - d_hot),  m_h = -(1 / beta) log sum_i exp(-beta d(pb_i, pb_h)) over the moved rows i with a
 *                  pseudo-beta;  Hub(v) = 0 (v <= 0), v^2 / 2 (0 < v < 1), v - 1/2 (v >= 1).  A hotspot row that is moved in the sample or
 *                  has no pseudo-beta, and a sample without a moved pseudo-beta, contribute exactly 0.
 *   energy[b][2] = sum_r weight_r * (Hub(d_r - hi_r) + Hub(lo_r - d_r)) over the restraints whose two atoms both exist
 *   grad_atom = dE/dx (B,L,14,3), exactly 0 on every row that is not moved;  grad_trans = sum_a g_a;
 *   grad_rot = sum_a (x_a - frame_trans) x g_a   (B,L,3) each, as in abx_clash_grad.
 * hotspots: H <= 64 row indices.  restr_idx: R <= 256 rows of {row_i, slot_i, row_j, slot_j}; restr_par: R rows of {lo, hi, weight}.
 * The *_host pointers are host copies of the same tables (required when H / R > 0): the argument checks read them before any launch;
 * the kernels read the device copies and skip an entry whose indices are out of range.
 * No atomics, fixed summation order; a sample's numbers do not depend on its neighbours in the batch.
 * The caller allocates the workspace (abx_contact_grad_workspace_bytes). */
typedef struct AbxContactArgs {
    const float* atom14; const unsigned char* atom_mask;   /* (B,L,14,3), (B,L,14) */
    const unsigned char* moved;                             /* (B,L) */
    const unsigned char* target;                            /* (L) */
    const float* frame_trans;                               /* (B,L,3) */
    const int* hotspots; const int* hotspots_host;          /* (H) */
    const int* restr_idx; const int* restr_idx_host;        /* (R,4) */
    const float* restr_par; const float* restr_par_host;    /* (R,3) */
    float w_contact, d0, d1, w_hot, d_hot, beta;
    float* energy;                                          /* (B,3): contact, hotspot, restraint */
    float* grad_atom; float* grad_trans; float* grad_rot;
    int B, L, H, R;
} AbxContactArgs;
long long abx_contact_grad_workspace_bytes(int B, int L, int H);
int abx_contact_grad(const AbxContactArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Design scores (SURVEY.md 8f-4 "eval metrics"): what the reference computes offline from the written PDB files, per structure of a
 * batch of B designs of ONE complex, on the device.  One row of ABX_SCORE_COLS float64 values per structure:
 *   0-13  {heavy,light}_cdr{1,2,3}_{AAR,RMSD} and heavy_cdr3_Loop_{AAR,RMSD} in the order of abx/common/ab_utils.py:124-167
 *         (calc_ab_metrics; abx_amd.metrics.SCORE_COLUMNS): ONE Kabsch superposition (abx/utils.py:444-465, the optimal proper
 *         rotation) of the antibody C-alpha (rows < Lab, slot 1) on the ground truth, then sqrt(mean |delta|^2) and the fraction of
 *         equal tokens over the rows whose cdr_def is 1 / 3 / 5 / 8 / 10 / 12; Loop = rows [4:-2] of the CDR-H3 rows in sequence order.
 *         A row whose ground-truth C-alpha does not exist is left out of the fit, the RMSD and the AAR (the Loop slice is taken
 *         before that); a region without rows gives NaN in both of its columns.  Centroids, covariance, rotation (Horn's quaternion
 *         form, Jacobi sweeps on the 4x4 matrix) and deviations are float64.
 *   14-16 n_viol_c_n, n_viol_ca_c_n, n_viol_c_n_ca: the sums of the three violation masks of between_residue_bond_loss
 *         (eval/metric_scripts/cal_vio.py:74-75, 93-94, 107-108) in its fp32 arithmetic; linked pairs as in AbxGuidanceArgs.
 *   17-18 n_clash, n_clash_inter: the number of atom pairs (each once) with d < r_a + r_b - overlap_tolerance under the pair rules of
 *         the clash energy of abx_clash_grad (the same fp32 expression: n_clash > 0 exactly when that energy is positive), and those
 *         of them whose atoms carry different chain ids.
 * The predicted structure: pred_atom14 (B, Lpred, 14, 3) with Lab <= Lpred <= L and the batch stride pred_sb (floats), pred_seq
 * (B, >= Lab) tokens with the batch stride pred_seq_sb; rows >= Lpred take their coordinates, rows >= Lab their residue type from the
 * ground truth (a sampler record holds the antibody only).  pred_mask (B, L, 14) is optional: NULL = an atom exists where the radius
 * table of its residue type is positive (rows >= Lpred: where the ground-truth atom exists).  res_mask (L) optional: 0 removes a
 * (padding) row from the violation and clash counts.
 * The complex: gt_atom14 (L,14,3), gt_exists (L,14), gt_seq (L), chain_id (L), residx (L, optional) shared by the B structures
 * (complex_batched = 0) or one per structure (complex_batched = 1: (B,L,...)); cdr_def (L) is always shared.
 * out: row b starts at out + b * out_stride (doubles, out_stride >= ABX_SCORE_COLS): successive calls can fill successive rows of
 * one table.  Two launches, no synchronisation, no allocation; the caller allocates the workspace
 * (abx_design_scores_workspace_bytes).  L > 1 as for abx_clash_grad. */
#define ABX_SCORE_COLS 19
typedef struct AbxDesignScoreArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const int* cdr_def; const int* chain_id;
    const int* residx;                              /* optional residue numbers */
    int complex_batched;
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs */
    float overlap_tolerance, bond_tolerance_factor;
    double* out; long long out_stride;
    int B, L, Lab;
} AbxDesignScoreArgs;
long long abx_design_scores_workspace_bytes(int B, int L);
int abx_design_scores(const AbxDesignScoreArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Violation relaxation of designed residues (the "relax" step between design and evaluation; upstream runs PyRosetta FastRelax,
 * relax_pdb.py / abx/relax.py, which this project does not use): steepest descent with an adaptive step on
 *   E = E_viol|M + k_restraint * sum_{r in M} |CA_r - CA_r(input)|^2
 * in the space of rigid-body motions of every movable residue (translation t, rotation about its C-alpha as a unit quaternion) plus
 * its side-chain chi angles.  E_viol|M is the energy of abx_clash_grad (the same fp32 expressions, pair rules and link rule)
 * restricted to the terms that touch a movable residue: atom pairs with at least one atom in M (pairs inside M once) and the
 * peptide terms of (l, l+1) when l or l+1 is in M.  Bond lengths and angles inside a residue never change; fixed rows never move.
 * Atoms are rebuilt from the INPUT coordinates at every evaluation: local = x_in - CA_in; chi_k (k = 1..4, where chi_axis has one and
 * both axis atoms exist) rotates the slots with rigid_group >= 3 + k about the axis through the two axis atoms; x = R local + CA_in + t.
 * Generalised gradient of a residue from the atom gradients g_a: g_t = sum g_a (+ the restraint), tau = sum (x_a - CA) x g_a,
 * g_chi_k = axis_k . sum_{a downstream of k} (x_a - p_k) x g_a.  Trial: t -= eta g_t, R <- exp(-eta tau / rho^2) R,
 * chi_k -= eta g_chi_k / rho^2; accepted when E_trial < E (eta *= grow) else dropped (eta *= shrink); ends after max_iter energy
 * evaluations or when E == 0.  E (fp64 sums of fp32 terms) never increases.  A structure without an accepted step is returned as
 * a copy of its input; rows outside M are always copies.
 * The structure and the complex are given as for abx_design_scores (pred_* rows < Lpred, ground truth beyond; pred_mask / res_mask /
 * residx optional; the complex is shared by the B structures).  movable: (L) bytes, shared by the batch; the first M set rows below
 * Lpred are the movable set (M: their number, counted by the caller once per complex).  chi_axis: [21][4][2] atom14 slots of the
 * second and third atom of every chi definition (-1: the residue type has no such chi); rigid_group: [21][14] rigid group of every
 * atom14 slot (4..7: moved by chi1..chi4).
 * out_atom14 (B, Lpred, 14, 3) with the batch stride out_sb (floats); report: ABX_RELAX_COLS doubles per structure (row stride
 * report_stride): E_clash, E_bond, E_angle of the input; E_clash, E_bond, E_angle, E_restraint of the output; evaluations used,
 * accepted steps, final eta, largest C-alpha displacement (abx_amd.relax.RELAX_COLUMNS).
 * max_iter = 0: one evaluation, out_atom14 = the input, and gen_grad (B, M, 10: g_t, tau, g_chi), when given, receives the generalised
 * gradient of the input state (with max_iter > 0 it receives that of the returned state).
 * One launch, one workgroup per structure, the structure's atom table resident in LDS: 232 L + 340 M + 1024 bytes must fit 160 KB
 * (L = 352 with up to 238 movable residues), a larger problem is an argument error.  Every sum has a fixed order: a structure's
 * result does not depend on its batch mates.  No allocation, no synchronisation; the workspace (abx_relax_workspace_bytes) is reserved
 * for a global-memory atom table and may be empty today. */
#define ABX_RELAX_COLS 11
typedef struct AbxRelaxArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const int* chain_id;
    const int* residx;                              /* optional residue numbers (L) */
    const unsigned char* movable;                   /* (L) */
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs */
    const int* chi_axis; const int* rigid_group;    /* [21][4][2], [21][14] */
    float overlap_tolerance, between_chain_factor, bond_tolerance_factor, w_clash, w_bond, w_angle;
    float k_restraint, eta0, rho, grow, shrink;
    int max_iter;
    float* out_atom14; long long out_sb;
    double* report; long long report_stride;
    float* gen_grad;                                /* optional (B,M,10) */
    int B, L, Lab, M;
} AbxRelaxArgs;
long long abx_relax_workspace_bytes(int B, int L, int M);
/* LDS bytes a structure of L rows with M movable ones needs (<= 163840 to be accepted) */
long long abx_relax_lds_bytes(int L, int M);
int abx_relax(const AbxRelaxArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Interface analysis of designs: the geometric half of what upstream takes from PyRosetta's InterfaceAnalyzerMover for every written
 * PDB and for the wild type (abx/metric.py:28-59, eval/traj_evaluate.py:242-261, the _energy.csv tables of eval/metric_scripts): buried
 * solvent-accessible surface (dSASA_int), interface residues (nres_int) and antibody-antigen contacts.  No energies (dG / ddG need a
 * force field, which this project does not have), no hydrogens.  One row of ABX_IFACE_COLS float64 values per structure of a batch
 * of B designs of ONE complex (abx_amd.interface.INTERFACE_COLUMNS).
 * Side A: the rows < Lab (antibody); side B: the rows >= Lab (the FEATURISED antigen: a cropped patch when the complex was cropped).
 * Atoms: the existing atom14 slots whose radius in `radius` is positive; inflated radius R_a = (double)r_a + probe.
 * Shrake-Rupley surface on the P unit vectors of `sphere` ((P,3) float64, 1 <= P <= 1024, built by the caller: the golden spiral
 * z = 1 - (2k+1)/P, r = sqrt(1 - z^2), phi = k pi (3 - sqrt 5); the kernel evaluates no trigonometry).  Point p of atom a is occluded
 * by atom b != a iff |c_a + R_a u_p - c_b|^2 < R_b^2, in float64 from the float32 coordinates, without fused multiply-add, in this order:
 *   px = (double)x_a + R_a * ux;  dx = px - (double)x_b;  d2 = (dx*dx + dy*dy) + dz*dz;  d2 < R_b * R_b
 * so the point counts are exact integers that a host evaluation of the same IEEE operations reproduces (abx_amd.interface.
 * interface_host).  Per atom: acc_alone = points occluded by no atom of its own side, acc_cplx = those of them occluded by no atom of
 * the other side either: one pass gives the complex and both separated partners.  Area of a count: 4 pi R_a^2 count / P.
 *   0 sasa_complex        sum area(acc_cplx), all atoms          6 n_res_int_antibody  side-A residues with an atom acc_alone > acc_cplx
 *   1 sasa_antibody       sum area(acc_alone), side A            7 n_res_int_antigen   the same, side B
 *   2 sasa_antigen        sum area(acc_alone), side B            8 n_res_int_region    the same, rows with region != 0
 *   3 dsasa_int           sum area(acc_alone - acc_cplx), all    9 n_contact           cross-side atom pairs with d^2 < cutoff^2 (float64,
 *   4 dsasa_antibody      the side-A part of 3                                         dx = (double)x_a - (double)x_b, the same order)
 *   5 dsasa_region        the part of 3 of rows with region != 0 10 n_contact_region   those of 9 whose side-A atom is in a region row
 *                                                                11 n_atoms            atoms counted
 * The structure and the complex are given as for abx_design_scores (pred_* rows < Lpred, ground truth beyond, residue types of rows
 * < Lab from pred_seq; pred_mask / res_mask optional: res_mask = 0 removes a row from both sides; the complex is shared by the B
 * structures).  No link rule enters: chain ids and residue numbers are not read.  region: (L) bytes shared by the batch, optional
 * (NULL: columns 5, 8 and 10 are 0).  out / out_stride as in AbxDesignScoreArgs (out_stride >= ABX_IFACE_COLS).
 * points: optional (B, L, 14, 2) int32, acc_alone and acc_cplx of every slot (0 for absent slots).
 * Three launches - the compacted atom table of every structure; the point counts, one wave per atom with the structure's table in
 * LDS (20 bytes per atom14 slot + 12 KB must fit 160 KB: L <= 541, a larger problem is an argument error); the fixed-order
 * reduction to the row - no atomics, no allocation, no synchronisation: a structure's row depends on nothing but its own inputs.
 * The caller allocates the workspace (abx_interface_scores_workspace_bytes). */
#define ABX_IFACE_COLS 12
typedef struct AbxInterfaceArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const unsigned char* region;                    /* optional (L) */
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs */
    const double* sphere; int P;                    /* (P,3) unit vectors */
    double probe, cutoff;                           /* probe radius (1.4), contact distance (4.0), Angstrom */
    double* out; long long out_stride;
    int* points;                                    /* optional (B,L,14,2) */
    int B, L, Lab;
} AbxInterfaceArgs;
long long abx_interface_scores_workspace_bytes(int B, int L, int P);
int abx_interface_scores(const AbxInterfaceArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Ensemble analysis of the N designs of ONE complex: what a design is to the other designs (how many different loops are these, which
 * are the same answer twice, which few go on to the expensive evaluation).  Two calls: all pairs, then clusters and a summary row.
 *
 * abx_ensemble_pairs.  The structures are given as for abx_design_scores: pred_atom14 (N, Lpred, 14, 3) f32 with the structure stride
 * pred_sb (floats; the [:, :Lab] view of a longer tensor is read in place), pred_seq (N, >= Lpred) int64 with the row stride
 * pred_seq_sb.  region: (>= Lpred) bytes shared by the batch; the first M set rows below Lpred are the compared residues (M: their
 * number, counted by the caller once per complex).  atoms: 1 = C-alpha only (atom14 slot 1), 4 = backbone N, CA, C, O (slots 0-3).
 * Points per structure P = M * atoms in residue order, 1 <= P <= ABX_ENS_MAX_POINTS.
 * planes: three (N, N) float64 planes, plane p at planes + p * plane_stride (plane_stride >= N * N doubles), each symmetric with a
 * zero diagonal:
 *   0 rmsd_fit    sqrt(sum_p |R (a_p - ca) - (b_p - cb)|^2 / P) with ca, cb the centroids and R the optimal PROPER rotation of the
 *                 centred sets (the Kabsch convention of abx/utils.py:444-465, no reflection): the difference in shape
 *   1 rmsd_frame  sqrt(sum_p |a_p - b_p|^2 / P), no superposition: all designs share the complex's frame, the difference in placement
 *   2 seq_diff    the number of compared rows whose tokens differ (an exact integer)
 * Arithmetic: float64 from the float32 coordinates; centroid of a structure, covariance and both deviations of a pair as sums over the
 * points in index order; R from Horn's quaternion matrix by cyclic Jacobi rotations (any eigenvector of a degenerate largest
 * eigenvalue is optimal: collinear and planar point sets give their well-defined RMSD); the deviation of plane 0 is summed in a second
 * pass over the points with R, never formed as G_a + G_b - 2 lambda (which cancels for close structures).  (i, j) with i < j is
 * computed once and written to both entries; a pair reads nothing but its two structures, so its value does not depend on N or on
 * its neighbours in the batch.  One launch, no atomics, no allocation, no synchronisation; the workspace is empty today
 * (abx_ensemble_pairs_workspace_bytes returns 0 and a NULL workspace is accepted).
 *
 * abx_ensemble_cluster.  planes / plane_stride: the three planes above (symmetric: row i is read as column i).  Clusters by the
 * Daura / GROMOS rule on plane `metric` (0 rmsd_fit, 1 rmsd_frame) with `cutoff`: the neighbours of i are the j != i with d[i][j] <=
 * cutoff; the unassigned design with the most unassigned neighbours (ties: the lowest index) becomes a centre and forms the next
 * cluster with them; repeated until none is left.  N <= ABX_ENS_MAX_N (the neighbour bits of all designs stay in the LDS of one
 * workgroup); a larger N is an argument error, nothing is truncated.
 * out: ABX_ENS_COLS doubles per design (row stride out_stride >= ABX_ENS_COLS; abx_amd.ensemble.ENSEMBLE_COLUMNS):
 *   0 cluster          cluster index in order of discovery   5 rmsd_frame_mean  over the other N - 1 designs
 *   1 is_centre        0 / 1                                 6 rmsd_frame_min
 *   2 n_neighbours     others within the cutoff on the       7 seq_diff_mean    mean number of differing compared residues
 *                      clustering plane (all designs)        8 n_same_seq       others with seq_diff == 0
 *   3 rmsd_fit_mean    over the other N - 1 designs          9 first_same_seq   lowest index with seq_diff == 0 to this design
 *   4 rmsd_fit_min                                                              (its own index: the first of its sequence)
 * Sums run over the other designs in index order; N = 1: means and minima are NaN, counts 0.  centres: (N) int32, the centres in
 * order of discovery, padded with -1; n_clusters: one int32.  One launch of two workgroups (the clusters; the summary rows, one
 * thread per design), no atomics, no allocation, no synchronisation. */
#define ABX_ENS_MAX_POINTS 512
#define ABX_ENS_MAX_N 1024
#define ABX_ENS_COLS 10
typedef struct AbxEnsemblePairsArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* region;                    /* (>= Lpred) */
    int atoms, M;
    double* planes; long long plane_stride;
    int N;
} AbxEnsemblePairsArgs;
long long abx_ensemble_pairs_workspace_bytes(int N, int P);
int abx_ensemble_pairs(const AbxEnsemblePairsArgs* a, void* workspace, hipStream_t stream);
typedef struct AbxEnsembleClusterArgs {
    const double* planes; long long plane_stride;
    int metric;
    double cutoff;
    double* out; long long out_stride;
    int* centres; int* n_clusters;
    int N;
} AbxEnsembleClusterArgs;
int abx_ensemble_cluster(const AbxEnsembleClusterArgs* a, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Distogram head of designs: what the network's own pair representation predicts about a design (abx/model/head.py:26-44,
 * DistogramHead.forward: x = proj(pair), logits = 0.5 (x + x^T); head.py:99-102, MetricDictHead: pred = sum softmax(logits)[..., :t+1]
 * with t = #{breaks <= cutoff}).  The projection is linear, so the OPERAND is symmetrised: zs[i][j] = 0.5f * (z[i][j] + z[j][i]) in fp32
 * (commutative: (i, j) and (j, i) hold equal bits), logits[i][j] = zs[i][j] W + b by the exact fp32 MFMA, k ascending.
 * z (B, L, L, ABX_DISTO_CHANNELS) fp32 contiguous, 16-byte aligned (representations['pair'] of a network call).
 * W: impl.distogram.proj.weight [64][192] packed once by the caller into MFMA B fragments, 16-byte aligned:
 *   W[(((k / 4) * 4 + n / 16) * 4 + k % 4) * 16 + n % 16] = weight[n][k]   (abx_amd.ops.distogram_pack_weight)
 * bias [64].  breaks [num_breaks = 63] ascending (linspace(first_break, last_break, 63)), sq_breaks their fp32 squares (host).
 *
 * abx_distogram_scores.  pb (B, L, 3) fp32 pseudo-beta coordinates of the designs; classes (L) bytes shared by the batch
 * (ABX_DISTO_ANTIBODY | ABX_DISTO_ANTIGEN | ABX_DISTO_DESIGNED); valid (B, L) bytes; cutoff (8.0).  Per ordered pair i != j of valid rows:
 *   d2 = (dx*dx + dy*dy) + dz*dz, dx = pb_i.x - pb_j.x, ... in fp32, every operation rounded on its own (the order of abx_prev_pos)
 *   bin_real = sum_k (d2 > sq_breaks[k]);  realised contact: d2 < cutoff * cutoff (fp32)
 *   p = softmax(logits) with max subtraction: e_k = expf(l_k - max) (the difference exact in float64, rounded to fp32 for expf),
 *   every sum after it in float64.  nll = -ln p[bin_real];  entropy = -sum p ln p;  p_contact as above;
 *   E[d] = sum p_k c_k, c_k = midpoint of bin k (breaks[k-1], breaks[k]], the two open end bins extended by half a step.
 * table: ABX_DISTO_COLS doubles per design (row stride table_stride; abx_amd.confidence.CONFIDENCE_COLUMNS), an empty set gives 0:
 *   0 nll_all               mean nll, all pairs                    5 entropy_region               mean entropy, i designed
 *   1 nll_antibody_antigen  i antibody, j antigen                  6 exp_contacts_region_antigen  sum p_contact, i designed, j antigen
 *   2 nll_region            i designed                             7 n_contacts_region_antigen    realised contacts in that set
 *   3 nll_region_antigen    i designed, j antigen                  8 p_on_contacts_region_antigen mean p_contact over those contacts
 *   4 dist_err_region       mean |E[d] - sqrt(d2)|, i designed,    9 n_pairs_region               pairs with i designed
 *                           bin_real < 63 (d within the last break)
 * rows: optional (B, L, 4) doubles per residue i: mean nll over its valid partners, sum_{j antigen} p_contact, realised antigen
 * contacts, mean entropy.  p_contact / exp_dist: optional (B, L, L) fp32 planes of every pair (validity not applied), exactly
 * symmetric.  rowsums: caller scratch of B * L * ABX_DISTO_ROWSUMS doubles, fully written by the first launch before the second
 * reads it.  Two launches: grid (L, B), a workgroup walks the j tiles of its row in ascending order (per-row float64 sums in tile
 * order, then lane order); one wave per design sums the rows in ascending i.  No atomics, no allocation, no synchronisation: the
 * bits of a design depend on neither B nor its place in the batch.
 *
 * abx_distogram_logits.  The same kernel body stores the logits (B, L, L, 64) fp32 instead of reducing them (the reference's
 * heads['distogram']['logits']; 4 * B * L * L * 64 bytes: for a few designs, not for a batch).  Reads z, W, bias, B, L only. */
#define ABX_DISTO_CHANNELS 192
#define ABX_DISTO_BINS 64
#define ABX_DISTO_COLS 10
#define ABX_DISTO_ROWSUMS 10
#define ABX_DISTO_ANTIBODY 1
#define ABX_DISTO_ANTIGEN 2
#define ABX_DISTO_DESIGNED 4
typedef struct AbxDistogramArgs {
    const float* z;
    const float* W; const float* bias;
    const float* breaks; const float* sq_breaks; int num_breaks;
    const float* pb;
    const unsigned char* classes; const unsigned char* valid;
    float cutoff;
    double* table; long long table_stride;
    double* rows;                                   /* optional (B,L,4) */
    float* p_contact; float* exp_dist;              /* optional (B,L,L) */
    double* rowsums;                                /* scratch (B,L,ABX_DISTO_ROWSUMS) */
    int B, L;
} AbxDistogramArgs;
int abx_distogram_scores(const AbxDistogramArgs* a, hipStream_t stream);
int abx_distogram_logits(const AbxDistogramArgs* a, float* logits, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Accuracy of designs against the crystal structure: the lDDT that pLDDT predicts (abx/model/utils.py:102-155, lddt, the target of
 * predicted_lddt_loss), the TM block of TMscoreHead (abx/model/head.py:116-141; Kabsch, TMscore, GDT of abx/utils.py:562-578,
 * 525-560, 703-763) and the recovery of the native antibody-antigen residue contacts (DockQ's Fnat).  One row of ABX_ACC_COLS
 * float64 values per structure of a batch of B designs of ONE complex (abx_amd.accuracy.ACCURACY_COLUMNS).
 * The design and the complex are given as for abx_design_scores (pred_* rows < Lpred, Lpred = Lab or L, ground truth beyond, residue
 * types of rows < Lab from pred_seq, clamped to 0..20; pred_mask NULL: the design's rows < Lpred have the atoms of their residue type,
 * `radius` [21][14] > 0; res_mask = 0 removes a row from both structures; the complex is shared by the B structures).  The wild type
 * is gt_atom14 / gt_exists / gt_seq.
 * Scored atoms: slot a of row i when it exists in the wild type and in the design and (the two tokens are equal or a <= 4: N, CA, C,
 * O, CB): a mutated residue is compared on its backbone and CB.  Atoms related by a side-chain symmetry (Asp OD1 / OD2, the Phe
 * ring, ...) are NOT renamed: a flipped ring counts as a deviation.
 * lDDT (Mariani et al. 2013): the ordered pair (p, q) of scored atoms of different rows is included iff d2_wild < radius * radius, and
 * preserved at t in {0.5, 1, 2, 4} iff fabs(sqrt(d2_wild) - sqrt(d2_design)) < t; all in float64 from the float32 coordinates, without
 * fused multiply-add:  dx = (double)x_p - (double)x_q;  d2 = (dx*dx + dy*dy) + dz*dz.  Classes: 0 all, 1 bb (both slots <= 4), 2 ca (both
 * slots == 1: upstream's lddt on the C-alpha).  Per row and class five integers (counts): n_pairs and n_preserved at 0.5, 1, 2, 4,
 * over the pairs with p in that row.  lDDT of a row = (sum_t n_preserved_t) / (4 n_pairs), NaN without pairs; of a row set the same
 * with both sums over its rows (pair-pooled, upstream's per_residue=False).
 * Native contacts: the (antibody row i < Lab, antigen row j >= Lab) pairs with any two existing atoms (of each structure's own
 * atoms and coordinates; the scored-atom rule does not apply) with d2 < contact * contact: bit 0 in the wild type, bit 1 in the design.
 * TM block: the rows with a wild-type C-alpha; optimal proper rotation of the centred sets (Horn's quaternion, cyclic Jacobi, float64);
 * d_i the distances after it, N their number: tm_score = mean 1 / (1 + (d_i / d0)^2), d0 = 1.24 cbrt(max(21, N) - 15) - 1.8;
 * gdt_ts / gdt_ha = #{(i, c): d_i <= c} / (4 N) over c in {1, 2, 4, 8} / {0.5, 1, 2, 4}; rmsd_ca = sqrt(sum d_i^2 / N).  N = 0: NaN.
 *   0 lddt_all         all rows                          11 rmsd_ca
 *   1 lddt_antibody    rows < Lab                        12 n_native           residue pairs with bit 0
 *   2 lddt_region      rows with region != 0             13 n_kept             with both bits
 *   3 lddt_bb_region   class bb, region rows             14 fnat               13 / 12, NaN at 0 native
 *   4 lddt_ca_all      class ca, all rows                15 n_new              with bit 1 only
 *   5 lddt_ca_region   class ca, region rows             16 n_native_region    columns 12, 13 and 14 over the pairs whose
 *   6 plddt_region     mean plddt over the region rows   17 n_kept_region      antibody row is a region row
 *   7 plddt_err_region mean |plddt_i - 100 lDDT-ca_i|    18 fnat_region
 *                      over the region rows with pairs   19 n_pairs_region     n_pairs of class all over the region rows
 *   8 tm_score   9 gdt_ts   10 gdt_ha                    20 n_atoms_scored
 * region: (L) bytes shared by the batch, optional (NULL: no row is a region row); a row removed by res_mask is no region row.
 * plddt: optional (B, L) fp32 with the row stride plddt_sb (NULL: columns 6 and 7 are NaN).  out / out_stride as in
 * AbxDesignScoreArgs (out_stride >= ABX_ACC_COLS).  rows: optional (B, L, 4) doubles: lDDT all, bb, ca and n_pairs of class all.
 * counts: optional (B, L, 3, 5) int32.  contacts: optional (B, Lab, L - Lab) bytes.
 * Two launches: grid (16-row tile, structure), one thread per row atom, the column tiles of both structures streamed through LDS,
 * 15 integer counters per thread, reduced to the row with integer LDS adds (contact bits: integer LDS or); one block per structure
 * for the superposition, the pooled sums and the row.  No floating-point atomics, every float sum in a fixed order, no allocation,
 * no synchronisation: the bits of a structure depend on nothing but its own inputs.  The caller allocates the workspace
 * (abx_accuracy_scores_workspace_bytes). */
#define ABX_ACC_COLS 21
typedef struct AbxAccuracyArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const unsigned char* region;                    /* optional (L) */
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs (> 0: the type has the slot) */
    const float* plddt; long long plddt_sb;         /* optional (B,L) */
    double lddt_radius, contact;                    /* inclusion radius (15.0), residue contact distance (5.0), Angstrom */
    double* out; long long out_stride;
    double* rows;                                   /* optional (B,L,4) */
    int* counts;                                    /* optional (B,L,3,5) */
    unsigned char* contacts;                        /* optional (B,Lab,L-Lab) */
    int B, L, Lab;
} AbxAccuracyArgs;
long long abx_accuracy_scores_workspace_bytes(int B, int L);
int abx_accuracy_scores(const AbxAccuracyArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Polar interface contacts of designs: the chemical columns upstream takes from InterfaceAnalyzerMover beside dG and dSASA
 * (hbonds_int, delta_unsatHbonds; abx/metric.py:28-59, eval/traj_evaluate.py:233-261) that need no force field: hydrogen bonds and salt
 * bridges across the interface, and the polar atoms that binding buries without giving them a partner.  Heavy atoms only (no
 * hydrogens, no energies, no His protonation, no water).  One row of ABX_POLAR_COLS float64 values per structure of a batch of B
 * designs of ONE complex (abx_amd.polar.POLAR_COLUMNS).
 * table: [21][14] int32 per (residue type, atom14 slot), built by the caller from the atom names (abx_amd.polar.polar_table):
 * ABX_POLAR_DONOR | ABX_POLAR_ACCEPTOR | ABX_POLAR_CATION | ABX_POLAR_ANION role bits, ABX_POLAR_ELEMENT (the name starts with N or O:
 * splits the buried area only), and in bits 8-11 the atom14 slot of one bonded heavy atom, the antecedent.  A POLAR ATOM is a slot
 * with a donor or acceptor bit whose slot and antecedent slot both exist; at most 5 per residue type (Arg: N, O, NE, NH1, NH2; a table
 * with more is cut to 5 L atoms per structure).
 * Every decision in float64 from the float32 coordinates, without fused multiply-add, in this order, so every count is an exact
 * integer that a host evaluation of the same IEEE operations reproduces (abx_amd.polar.polar_host).  Per unordered pair (a, b) of
 * polar atoms of DIFFERENT rows, a before b in (row, slot) order:
 *   dx = (double)x_b - (double)x_a (likewise y, z);  d2 = (dx*dx + dy*dy) + dz*dz
 * Hydrogen bond (one a donor, the other an acceptor):  hb_min*hb_min <= d2 <= hb_max*hb_max  and, with u = ante_a - a, v = ante_b - b
 * (component-wise in float64),
 *   ta = (u.x*dx + u.y*dy) + u.z*dz;  uu = (u.x*u.x + u.y*u.y) + u.z*u.z;  ta <= 0  and  ta*ta >= cos2 * (uu * d2)
 *   tb = (v.x*dx + v.y*dy) + v.z*dz;  vv likewise;                         tb >= 0  and  tb*tb >= cos2 * (vv * d2)
 * i.e. both angles antecedent - atom ... partner are at least hb_angle (90 degrees: the HBPLUS heavy-atom rule).  hb_angle in
 * [90, 180) degrees; hb_cos2 = cos^2(hb_angle) is computed by the caller (checked here to 1e-12; exactly 0 is used at 90 degrees): no
 * square root, no trigonometry on the device.  The test is symmetric under exchange of a and b bit for bit.  No link rule: the
 * backbone C-O ... N(i+1) angle is about 30 degrees and fails; chain ids and residue numbers are not read.
 * Salt bridge: a pair of rows on DIFFERENT sides counts once when a cation atom of one and an anion atom of the other have
 * d2 <= salt*salt, however many atom pairs qualify.
 * Burial, from `points` ((B, L, 14, 2) int32: acc_alone, acc_cplx of every slot, the output of abx_interface_scores for the same
 * structures with P sphere points and `probe`): a polar atom is AT THE INTERFACE if acc_alone > acc_cplx, BURIED BY BINDING if
 * acc_alone > 0 and acc_cplx == 0, UNSATISFIED if buried by binding and in no hydrogen bond (same side or cross).  Area of a count:
 * 4 pi R_a^2 count / P, R_a = (double)r_a + probe, over the existing slots with a positive radius.
 *   0 n_hbond_int           bonds between side A and side B         7 n_polar_buried  polar atoms buried by binding
 *   1 n_hbond_int_bb        those of 0 between two backbone atoms   8 n_unsat         buried and unsatisfied
 *                           (slots 0-3)                             9 n_unsat_region  those of 8 in region rows
 *   2 n_hbond_region        those of 0 with an atom in a region row 10 dsasa_polar    area(acc_alone - acc_cplx), ABX_POLAR_ELEMENT slots
 *   3 n_hbond_intra_region  same-side bonds with an atom in a       11 dsasa_apolar   the same over all other atoms (10 + 11 = dsasa_int)
 *                           region row                              12 n_hbond_total  all bonds of the structure
 *   4 n_salt_int            cross-side salt-bridged row pairs       13 n_polar        polar atoms counted
 *   5 n_salt_region         those of 4 with a region row
 *   6 n_polar_int           polar atoms at the interface
 * points NULL: columns 6-11 are -1 (P and probe are not read).  region NULL: columns 2, 3, 5 and 9 are 0.
 * The structure and the complex are given as for abx_interface_scores (pred_* rows < Lpred, ground truth beyond, residue types of rows
 * < Lab from pred_seq; pred_mask / res_mask optional; side A = rows < Lab; region (L) bytes shared by the batch).
 * bonds: optional (B, L, 14, 2) int32, the same-side and cross-side bonds of every slot (0 for absent or non-polar slots; its sum over
 * a structure is 2 x column 12).  rows: optional (B, L, 4) int32 per row: its cross-side bonds, its same-side bonds, the rows it is
 * salt-bridged to across the interface (sum: 2 x column 4), its unsatisfied atoms (-1 without points).
 * One launch, one workgroup per structure: the polar atoms compacted in slot order into LDS (216 bytes per row + 512 must fit 160 KB:
 * L <= 756, a larger problem is an argument error), the pairs dealt to the waves in a fixed pattern, integer LDS atomics for the
 * counters (integers commute), the two areas in a fixed order.  No global atomics, no allocation, no synchronisation: a structure's
 * row depends on nothing but its own inputs.  The workspace is empty today (abx_polar_scores_workspace_bytes returns 0 and a NULL
 * workspace is accepted). */
#define ABX_POLAR_COLS 14
#define ABX_POLAR_DONOR 1
#define ABX_POLAR_ACCEPTOR 2
#define ABX_POLAR_CATION 4
#define ABX_POLAR_ANION 8
#define ABX_POLAR_ELEMENT 16
typedef struct AbxPolarArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const unsigned char* region;                    /* optional (L) */
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs */
    const int* table;                               /* [21][14] roles | antecedent slot << 8 */
    const int* points; int P; double probe;         /* optional (B,L,14,2) of abx_interface_scores, its P and probe */
    double hb_min, hb_max;                          /* donor-acceptor distance range (2.0, 3.5), Angstrom */
    double hb_angle, hb_cos2;                       /* smallest antecedent-atom-partner angle (90.0 degrees) and its squared cosine */
    double salt;                                    /* cation-anion distance (4.0), Angstrom */
    double* out; long long out_stride;
    int* bonds;                                     /* optional (B,L,14,2) */
    int* rows;                                      /* optional (B,L,4) */
    int B, L, Lab;
} AbxPolarArgs;
long long abx_polar_scores_workspace_bytes(int B, int L);
/* LDS bytes a structure of L rows needs (<= 163840 to be accepted) */
long long abx_polar_scores_lds_bytes(int L);
int abx_polar_scores(const AbxPolarArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Developability of designs: spatial aggregation propensity (SAP, Chennamsetty et al. 2009), chain charges and sequence liabilities of
 * the FREE antibody, rows < Lab (the antigen enters only through acc_alone, the antibody's surface with the antigen taken away).  One
 * row of ABX_DEV_COLS float64 values per structure of a batch of B designs of ONE complex (abx_amd.developability.
 * DEVELOPABILITY_COLUMNS).  No pI, no patch metrics, no hydrogens; His carries no charge.
 * The structure and the complex are given as for abx_polar_scores (pred_* rows < Lpred, residue types of rows < Lab from pred_seq,
 * clamped to 0..20; pred_mask / res_mask optional; region (L) bytes shared by the batch, optional), with chain_id (L), residx (L,
 * optional) and cdr_def (L) as for abx_design_scores.  points: (B, L, 14, 2) int32, the output of abx_interface_scores for the same
 * structures with P sphere points; only acc_alone (points[..., 0]) is read.
 * COUNTED ATOMS: the slots of rows < Lab that exist and have radius > 0.  A row is PRESENT if it has a counted atom.
 * Tables of the caller (abx_amd.developability.weight_table), per (residue type, atom14 slot): a [21][14] doubles, the area of one sphere
 * point, 4 pi (r + probe)^2 / P; ref [21] doubles, the side-chain area of the isolated residue (0: Gly, X); q [21][14] int64, the
 * fixed-point weight of one accessible point, rint(2^30 a h / ref), 0 on slots < 4 (the kernel knows no hydrophobicity scale).
 * q_max: the largest |q| of the table.
 *   w_j   = acc_alone_j * q[type_j][slot_j]                                                     (int64)
 *   SAP_i = sum of w_j over the counted atoms j with (dx*dx + dy*dy) + dz*dz <= radius2, j = i included;  dx = (double)x_j - (double)x_i
 *           (likewise y, z) in float64 without fused multiply-add                                (int64: the order does not matter)
 * EXPOSED row: ref[type] > 0 and rel >= exposed * ref[type], rel = sum over the slots s = 4..13 in slot order of (double)acc_alone_s *
 * a[type][s] (0 for a slot that is not counted).  LINKED rows r - 1, r: both present, the same chain_id and (residx given)
 * residx[r] == residx[r-1] + 1.  Heavy chain: the chain_id of row 0; light: every other chain id of the rows < Lab.  CDR rows: cdr_def
 * in {1, 3, 5, 8, 10, 12}.  A liability belongs to its first row (the N, D, M, W or C).
 *   0 sap_pos              sum of max(SAP_i, 0) / 2^30              10 n_glyc        N-x-[ST], x != P, three linked rows, N exposed
 *   1 sap_pos_cdr          the same over atoms of CDR rows          11 n_deamid      N-[GS], two linked rows, N exposed
 *   2 sap_pos_region       the same over atoms of region rows       12 n_isomer      D-[GS], D exposed
 *   3 sap_max_res          max over present rows of                 13 n_frag        D-P, D exposed
 *                          (row's sum of SAP_i / its atoms) / 2^30  14 n_met_ox      exposed Met
 *   4 n_res_sap_pos        rows whose sum of SAP_i > 0              15 n_trp_ox      exposed Trp
 *   5 n_res_sap_pos_region those in the region                      16 n_cys_free    Cys with a counted SG and no other counted SG of the
 *   6 charge_heavy         (K + R) - (D + E), present heavy rows                     antibody with d2 <= 6.25 (2.5 A); no exposure rule
 *   7 charge_light         the same for the light rows              17 n_liab        sum of 10-16
 *   8 charge_product       column 6 x column 7                      18 n_liab_region those whose first row is a region row
 *   9 n_his                His among the present rows               19 n_liab_cdr    those whose first row is a CDR row
 *                                                                   20 n_atoms       counted atoms
 * The divisions are float64 divisions of the exact integers converted to float64 (row sum / atom count, then / 2^30).  Without a present
 * row column 3 is 0.
 * rows: optional (B, L, 4) doubles per row: mean SAP of its atoms (column 3's quantity), rel / ref[type] (0 where ref is 0), the
 * liability mask (bit k: the row starts a liability of column 10 + k), the charge (+1, -1, 0); rows >= Lab and absent rows are 0.
 * Bounds: |w_j| <= P q_max.  With the shipped tables P q_max < 0.5 * 2^30 at P = 128 ... 1024 (q shrinks as P grows; a coarse surface of
 * a few points has coarse reference areas and up to three times that, which is why q_max is an argument), at most 10 weighted and 14
 * counted atoms per row: |SAP_i| < 5 * 2^30 Lab and a structure's sum < 70 * 2^30 Lab^2 in the worst case (every atom fully exposed and
 * within the radius of every other), below 2^53 - the division by 2^30 is exact - up to Lab = 346 at P = 1024 as at P = 128; real
 * antibodies stay four orders of magnitude below (7 10^11 at Lab = 231).  A problem with 140 P q_max Lab^2 >= 2^63 could leave int64 and
 * is an argument error, as is Lab > 2048 (the row tables of the last kernel live in LDS).
 * Three launches: (1) one workgroup per structure weighs the counted atoms and compacts them into the workspace, all of them as the
 * i-list, those with w != 0 as the j-list; (2) grid (tile of 256 i-atoms, structure): one thread per atom i, the j-list through LDS in
 * chunks of j_chunk atoms (0: the default of 2048, 40 KB; 1..2048 otherwise - it exists so that a test can force several chunks on a
 * small complex), every lane reads the same j (a broadcast), SAP_i goes to the workspace; (3) one workgroup per structure for the row
 * sums, the counts and the row.  Integer LDS atomics only, no global atomics, no allocation, no synchronisation: a structure's row
 * depends on nothing but its own inputs.  The caller allocates the workspace (abx_developability_scores_workspace_bytes). */
#define ABX_DEV_COLS 21
typedef struct AbxDevelopabilityArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const unsigned char* region;                    /* optional (L) */
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs */
    const int* chain_id; const int* residx;         /* (L); residx optional */
    const int* cdr_def;                             /* (L) */
    const long long* q; long long q_max;            /* [21][14] fixed-point weights of a sphere point, the largest |q| */
    const double* a; const double* ref;             /* [21][14] area of a sphere point, [21] reference side-chain areas */
    const int* points; int P;                       /* (B,L,14,2) of abx_interface_scores and its P */
    double radius2;                                 /* squared radius of the SAP sphere (100.0), square Angstrom */
    double exposed;                                 /* smallest relative side-chain area of an exposed residue (0.075), in [0, 1] */
    double* out; long long out_stride;
    double* rows;                                   /* optional (B,L,4) */
    int j_chunk;                                    /* 0: the default */
    int B, L, Lab;
} AbxDevelopabilityArgs;
long long abx_developability_scores_workspace_bytes(int B, int L);
int abx_developability_scores(const AbxDevelopabilityArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Shape complementarity of designs: the Sc statistic of Lawrence & Colman (1993), upstream's sc_value of InterfaceAnalyzerMover, on the
 * CONTACT part of the molecular (Connolly) surface of each separated partner.  One row of ABX_SHAPE_COLS float64 values per structure of
 * a batch of B designs of ONE complex (abx_amd.shape.SHAPE_COLUMNS).  No re-entrant (toroidal / concave) patches, no hydrogens; the
 * antigen is the featurised patch; the value rises with the dot density P.
 * Structure, sides, atoms and radii exactly as for abx_interface_scores: pred_* / gt_* / pred_mask / res_mask / region, side A = rows
 * < Lab, side B = rows >= Lab, the atoms are the existing atom14 slots with a positive radius, sphere = P unit vectors (float64), probe.
 * points: (B, L, 14, 2) int32, REQUIRED: the output of abx_interface_scores for the same structures, sphere and probe.  It names the
 * atoms that are processed - those with acc_alone > acc_cplx - and fixes every list size and offset before a dot is generated.
 * DOTS.  A dot is (atom a, point p).  Its surface point is s = c_a + R_a u_p with R_a = (double)r_a + probe, computed as for the interface
 * (px = xa + R_a * ux: multiply, then add); an atom b occludes s iff (dx*dx + dy*dy) + dz*dz < R_b * R_b, dx = px - (double)x_b.  The dot
 * is ON THE SURFACE of its side iff no other atom of its own side occludes s, BURIED iff in addition an atom of the other side occludes
 * s, OPEN iff on the surface and not buried.  Its position is m = c_a + r_a u_p: mx = (double)x_a + (double)r_a * ux (multiply, then
 * add, no contraction); its normal is u_p.
 * LISTS of side X, in (row, slot, p) ascending order: I_X = its buried dots; E_X = the open dots of those atoms of X that own at least one
 * buried dot.  |I_X| = sum of (acc_alone - acc_cplx), |E_X| = sum of acc_cplx over the processed atoms of X.
 * TRIMMING (Lawrence & Colman's peripheral band): a dot i of I_X is kept iff no e of E_X has (dx*dx + dy*dy) + dz*dz < trim * trim,
 * dx = mx_i - mx_e.  trim = 0 keeps every dot.  T_X = the kept dots, in order.
 * MATCH: for i in T_X, j = the dot of T_Y (the other side) with the smallest d2 = (dx*dx + dy*dy) + dz*dz, dx = mx_i - mx_j; ties go to the
 * lowest list index.  S_i = -((ux_i*ux_j + uy_i*uy_j) + uz_i*uz_j) * exp(-(weight * d2)).
 * MEDIAN of n values sorted ascending: v[(n-1)/2] for odd n, (v[n/2-1] + v[n/2]) * 0.5 for even n, 0 for n = 0 or an empty T_Y.
 *   0 sc                  (column 1 + column 2) * 0.5        6 n_dots_antibody     |T_A|
 *   1 sc_antibody         median S over T_A                  7 n_dots_antigen      |T_B|
 *   2 sc_antigen          median S over T_B                  8 n_dots_region       dots of T_A in rows with region != 0
 *   3 sc_region           median S over the dots of T_A      9 n_trimmed_antibody  |I_A| - |T_A|
 *                         in rows with region != 0          10 n_trimmed_antigen   |I_B| - |T_B|
 *   4 gap_antibody        sqrt(median d2 over T_A)
 *   5 gap_antigen         sqrt(median d2 over T_B)
 * CAPACITY.  max_dots: the capacity of each of the four lists (I_A, I_B, E_A, E_B) of a structure.  A structure whose sizes from
 * `points` exceed it gets a row of eleven -1; so does a structure with an atom whose recomputed counts disagree with `points`
 * (or whose `points` name an atom that does not exist, or hold counts outside 0 <= acc_cplx <= acc_alone <= P).  The dot kernel never
 * writes past the segment `points` promised.
 * Five launches: (1) one workgroup per structure: atom table, interface atoms, prefix sums of their dot counts in atom order; (2) one
 * wave per interface atom, the atom table in LDS (L <= 541), the point test of the interface kernel, the dots to their segments by
 * ballot prefix sums; (3) one workgroup per (side, structure): trimming, E through LDS in chunks, the kept dots compacted in place;
 * (4) grid (at most 8 workgroups walking tiles of 256 kept dots, side, structure): one thread per dot, the other side's kept dots through
 * LDS in chunks of j_chunk (0: the default of 1024; 1..1024 otherwise - it exists so that a test can force ragged chunks); (5) one
 * workgroup per structure: the medians by radix select, the row.  Integer LDS atomics only, no global atomics, no allocation, no
 * synchronisation: a structure's row depends on nothing but its own inputs.  The caller allocates the workspace
 * (abx_shape_scores_workspace_bytes: per structure 64 + 504 L + 144 max_dots bytes, rounded up to 16). */
#define ABX_SHAPE_COLS 11
typedef struct AbxShapeArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const unsigned char* region;                    /* optional (L) */
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs */
    const double* sphere; int P;                    /* (P,3) unit vectors, 1 <= P <= 1024 */
    const int* points;                              /* (B,L,14,2) of abx_interface_scores for these structures, sphere and probe */
    double probe;                                   /* probe radius (1.4), Angstrom */
    double trim;                                    /* width of the peripheral band (1.5), Angstrom, >= 0 */
    double weight;                                  /* of d2 in the exponent (0.5), 1 / square Angstrom, >= 0 */
    double* out; long long out_stride;
    int max_dots;                                   /* capacity of each dot list of a structure (8192), 1..1048576 */
    int j_chunk;                                    /* 0: the default */
    int B, L, Lab;
} AbxShapeArgs;
long long abx_shape_scores_workspace_bytes(int B, int L, int P, int max_dots);
int abx_shape_scores(const AbxShapeArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Surface patches of designs: three of the five numbers of the Therapeutic Antibody Profiler (Raybould et al. 2019) - the patches of
 * surface hydrophobicity (PSH), of positive (PPC) and of negative charge (PNC) - with its Fv charge symmetry parameter (SFvCSP) and its
 * CDR length on the FREE antibody (rows < Lab), and the charge pairing ACROSS the interface out to the same cutoff.  One row of
 * ABX_PATCH_COLS float64 values per structure of a batch of B designs of ONE complex (abx_amd.patches.PATCHES_COLUMNS).  Not the TAP
 * server's numbers: the exposure reference is the isolated-residue area of abx_developability_scores, the CDRs are cdr_def as given (no
 * +-2 anchors), no hydrogens, no pI.
 * The structure and the complex are given as for abx_developability_scores (pred_* rows < Lpred, residue types of rows < Lab from
 * pred_seq, clamped to 0..20; pred_mask / res_mask optional; region (L) bytes shared by the batch, optional; chain_id, cdr_def (L)).
 * points: (B, L, 14, 2) int32, the output of abx_interface_scores for the same structures; only acc_alone (points[..., 0]) is read.
 * COUNTED ATOMS: the slots of ANY row that exist and have radius > 0.  A row is PRESENT if it has a counted atom.  Coordinates must be
 * finite.  Float32 coordinates are converted to float64; no operation is fused.
 * Tables of the caller: h [21] doubles, the hydrophobicity of a residue type (abx_amd.patches.kyte_doolittle: 1..2, X = 0) and h_max,
 * the largest |h|; q10 [21] int32, its charge in tenths (abx_amd.patches.charge_table: K, R +10, D, E -10, H +1) and q_max, the largest
 * |q10|; table [21][14] int32, the role bits of abx_polar_scores, of which ABX_POLAR_CATION and ABX_POLAR_ANION are read; a [21][14]
 * and ref [21] doubles as for abx_developability_scores; gly: the residue type whose h a salt-bridged row takes.
 *   1. EXPOSED row i < Lab: present, ref[type] > 0 and rel >= exposed * ref[type], rel as for abx_developability_scores (a type without
 *      a reference area - Gly, X - is never exposed).
 *   2. D2[i][j], i < Lab, j < L, j != i: the minimum over the counted atoms a of i and b of j of (dx*dx + dy*dy) + dz*dz,
 *      dx = (double)x_b - (double)x_a (likewise y, z); +inf if either row has none.  S2[i][j]: the same minimum over the atom pairs of
 *      which one has the CATION bit and the other the ANION bit.  Both are symmetric bit for bit.
 *   3. SALT-BRIDGED row i < Lab: some j < Lab, j != i, has S2[i][j] <= salt2.
 *   4. SEED: exposed and cdr_def in {1, 3, 5, 8, 10, 12}.  VICINITY: exposed, and a seed or with D2[i][s] <= vicinity2 to a seed s != i.
 *   5. h_eff = h[gly] for a salt-bridged row, h[type] otherwise.  Q = (double)q10[type] / 10.0.
 *   6. Over the pairs i < j < Lab, both in the vicinity, D2 <= cutoff2:  r2 = max(D2, 1.0) (two coincident atoms keep the term bounded);
 *      psh_q += llrint(2^30 * ((h_eff_i * h_eff_j) / r2));  c = llrint(2^30 * (fabs(Q_i * Q_j) / r2));  ppc_q += c if both q10 > 0,
 *      pnc_q += c if both q10 < 0.  The *_region sums take the pairs with region[i] | region[j].
 *   7. sfvcsp = (double)(sum of q10 over the exposed rows with chain_id == chain_id[0]  x  sum over the other exposed rows) / 100.0.
 *   8. Over the pairs i < Lab <= j, both present, q10_i * q10_j != 0, D2 <= cutoff2 (no exposure rule): the same c; opposite signs go
 *      to cross_attract, equal signs to cross_repel; the *_region sums take the pairs with region[i].
 *   0 psh         psh_q / 2^30              7 cross_attract          11 n_cdr           present rows < Lab with a CDR code
 *   1 ppc         ppc_q / 2^30              8 cross_repel            12 n_exposed       exposed rows
 *   2 pnc         pnc_q / 2^30              9 cross_attract_region   13 n_vicinity      rows in the vicinity
 *   3 sfvcsp                               10 cross_repel_region     14 n_pairs         pairs of 6
 *   4 psh_region, 5 ppc_region, 6 pnc_region                         15 n_salt          salt-bridged rows in the vicinity
 *                                                                    16 n_cross, 17 n_cross_region   pairs of 8
 * rows: optional (B, L, 4) doubles per row: the sum of its psh terms / 2^30, of its ppc or pnc terms / 2^30 (a row has one sign), its
 * cross_attract minus its cross_repel terms / 2^30 (antigen rows too), and its flags: 1 present, 2 exposed, 4 seed, 8 vicinity,
 * 16 salt-bridged, 32 region (0 for an absent row).
 * Bounds: a term is at most 2^30 h_max^2 (2^32 with the shipped table), a cross term at most 2^30 (q_max / 10)^2, over at most Lab^2 / 2
 * and Lab (L - Lab) pairs: with L <= 2048 every sum stays below 2^53 and its division by 2^30 is exact.  A problem with
 * 2^30 h_max^2 Lab^2 or 2^30 (q_max / 10)^2 Lab L >= 2^62 could leave int64 and is an argument error, as is L > 2048 (the row tables
 * of the last kernel live in LDS).
 * Three launches: (1) one workgroup per structure: type, presence, exposure, seed and region of every row, its counted atoms compacted
 * to the front of its 14 float4 (x, y, z, role bits) in the workspace; (2) grid (tile of 256 j-rows, tile of 16 i-rows, structure): one
 * lane per j-row with its atoms in registers as float64, the atoms of the i-rows broadcast from LDS; D2 to a (Lab, L) float64 plane of
 * the workspace, the salt bit of a j-row against the tile to a byte; (3) one workgroup per structure: salt-bridged rows, vicinity, the
 * terms, the row.  Integer LDS atomics only, no global atomics, no allocation, no synchronisation: a structure's row depends on nothing
 * but its own inputs.  The caller allocates the workspace (abx_patch_scores_workspace_bytes). */
#define ABX_PATCH_COLS 18
typedef struct AbxPatchArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const unsigned char* region;                    /* optional (L) */
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs */
    const int* points;                              /* (B,L,14,2) of abx_interface_scores */
    const int* chain_id;                            /* (L) */
    const int* cdr_def;                             /* (L) */
    const double* h; double h_max;                  /* [21] hydrophobicity of a residue type, the largest |h| */
    const int* q10; int q_max;                      /* [21] charge of a residue type in tenths, the largest |q10| */
    const int* table;                               /* [21][14] role bits of abx_polar_scores */
    const double* a; const double* ref;             /* [21][14] area of a sphere point, [21] reference side-chain areas */
    double cutoff2, vicinity2, salt2;               /* squared distances of a pair (56.25), of the vicinity (16.0), of a salt bridge (10.24) */
    double exposed;                                 /* smallest relative side-chain area of an exposed residue (0.075), in [0, 1] */
    double* out; long long out_stride;
    double* rows;                                   /* optional (B,L,4) */
    int gly;                                        /* the residue type whose h a salt-bridged row takes */
    int B, L, Lab;
} AbxPatchArgs;
long long abx_patch_scores_workspace_bytes(int B, int L, int Lab);
int abx_patch_scores(const AbxPatchArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Torsion analysis of designs: the backbone dihedrals between the residues (phi, psi, omega - cis and twisted peptides, phi >= 0, the
 * ABEGO class) and the chi angles against the crystal structure (chi1 / chi1+2 recovery).  No upstream file:line: the reference has no
 * such analysis (its torsions exist as network features only, abx/model/atom.py); the definitions are the ones written here.  One row
 * of ABX_TORSION_COLS float64 values per structure of a batch of B designs of ONE complex (abx_amd.torsions.TORSIONS_COLUMNS).  No
 * Ramachandran probability surface, no hydrogens, no chirality check; the chi of a mutated residue is not compared.
 * The design and the complex are given as for abx_accuracy_scores (pred_* rows < Lpred, Lab <= Lpred <= L, residue types of rows < Lab
 * from pred_seq, clamped to 0..20; pred_mask (B,L,14) NULL: a row has the atoms of its residue type, `radius` [21][14] > 0; res_mask = 0
 * removes a row from both structures).  Only the rows < Lab are read: the antigen is not.  The wild type is gt_atom14 / gt_exists /
 * gt_seq.  chain_id (L); residx (L) optional.  region: (L) bytes, optional (NULL: no row is a region row).
 * LINK (i-1, i), 1 <= i < Lab: chain_id equal, residx consecutive when given (the rule of abx_design_scores), and N, CA, C present in
 * both rows.  Distance is not asked: a broken bond still has an omega.
 * DIHEDRAL of a, b, c, d, float64 from the float32 coordinates, no operation fused, sums as bracketed:
 *   b1 = b - a, b2 = c - b, b3 = d - c;  n1 = b1 x b2, n2 = b2 x b3  (n_x = u_y*v_z - u_z*v_y, ...);
 *   x = (n1x*n2x + n1y*n2y) + n1z*n2z;  y = sqrt((b2x*b2x + b2y*b2y) + b2z*b2z) * ((b1x*n2x + b1y*n2y) + b1z*n2z);
 *   r = sqrt(x*x + y*y);  angle = atan2(y, x) in degrees (reported only: no decision reads it).
 *   omega_i = (CA, C of i-1; N, CA of i) and phi_i = (C of i-1; N, CA, C of i) with link (i-1, i); psi_i = (N, CA, C of i; N of i+1)
 *   with link (i, i+1); chi_k of a row: the four atom14 slots chi_atoms[type][k] (< 0: the type has no chi_k), all present.
 * DECISIONS, on (x, y, r) and the (cos, sin) pairs of the caller (computed once on the host, so that a twin uses the same bits):
 *   negative(angle):      y < 0
 *   wider(angle, h):      x <= h[0] * r                                    |angle| >= h
 *   within(angle, m, h):  x*m[0] + y*m[1] >= h[0] * r                      |angle - m| <= h
 *   cis = !wider(omega, cis);  twisted = wider(omega, cis) && !wider(omega, trans);  phi_pos = !negative(phi) and the type is not gly.
 *   ABEGO code of a row with phi, psi and omega: 5 (O) if !wider(omega, o); else 1 (A) if negative(phi) and within(psi, a_mid, a_half);
 *   else 2 (B) if negative(phi); else 3 (G) if x_psi >= g_half[0] * r_psi (|psi| <= 100); else 4 (E).  0: undefined.  (An interval
 *   is closed at both ends here; the half-open statement differs on a set of measure zero, which a twin counts as borderline.)
 *   The shipped pairs: cis 30, trans 150, o 90, a_mid -12.5, a_half 62.5, g_half 100 degrees, chi_tol 40 (abx_amd.torsions.thresholds).
 * DIFFERENCE of an angle of the design (x, y) and of the wild type (u, v):  c = x*u + y*v;  s = y*u - x*v;  for a chi with
 *   chi_pi[type][k] != 0 (a symmetric end: Asp chi2, Glu chi3, Phe / Tyr chi2) c = fabs(c);  |delta| = atan2(fabs(s), c) in degrees;
 *   ok = c >= chi_tol[0] * sqrt(c*c + s*s).
 * A chi is COMPARED in a region row whose two tokens are equal when it is defined in both structures.
 *   0 n_links          links of the design                   13 abego_O
 *   1 cis              2 cis_nonpro (row i is not pro)       14 n_abego         region rows with a code in both structures
 *   3 twisted                                                15 abego_same      ... and the same code
 *   4 n_links_region   links with region[i-1] | region[i]    16 dphi_region     mean |delta phi| over the region rows with phi in both
 *   5 cis_region       6 twisted_region                      17 dpsi_region     18 domega_region     likewise
 *   7 phi_pos          8 phi_pos_region (region[i])          19 dbb_max_region  the largest |delta phi| or |delta psi| of 16, 17
 *   9 abego_A  10 abego_B  11 abego_G  12 abego_E            20 n_chi1  21 chi1_ok   rows with chi1 compared / ok
 *     (9-13: the region rows of the design by code)          22 n_chi12 23 chi12_ok  rows with chi1 and chi2 compared / both ok
 *                                                            24 chi_mae_region  mean |delta chi| over all compared chi
 *   16-19 and 24 are NaN where nothing is comparable.
 * rows: optional (B, Lab, 8) doubles: phi, psi, omega of the preceding link, chi1..chi4 in degrees (NaN: undefined) and the flag word
 * code | 8 cis | 16 twisted | 32 phi_pos | 64 region | 128 chi1 compared | 256 chi1 ok.  classes: optional (B, Lab) int32, the codes.
 * out / out_stride as in AbxDesignScoreArgs (out_stride >= ABX_TORSION_COLS).
 * One launch, one workgroup of 256 per structure, one lane per row (strided): N, CA, C of the wild type are staged as float64 in LDS
 * (72 Lab bytes, dynamic) and every row's seven (x, y) pairs and code go to the workspace (16 doubles a row, written and read back by
 * the same lane); then the design is staged the same way and measured against them.  Integer LDS counters, the four float sums in a
 * fixed order, the maximum as an integer LDS maximum of the bit pattern: a structure's row depends on nothing but its own inputs.
 * Lab <= ABX_TORSION_MAX_LAB (the LDS image stays below 64 KiB); more is an argument error.  No allocation, no synchronisation.  The
 * caller allocates the workspace (abx_torsion_scores_workspace_bytes). */
#define ABX_TORSION_COLS 25
#define ABX_TORSION_MAX_LAB 800
typedef struct AbxTorsionArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const unsigned char* region;                    /* optional (L) */
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs (> 0: the type has the slot) */
    const int* chain_id;                            /* (L) */
    const int* residx;                              /* optional (L) */
    const int* chi_atoms;                           /* [21][4][4] atom14 slots of chi_k of a residue type, < 0: no such chi */
    const unsigned char* chi_pi;                    /* [21][4] != 0: chi_k is compared modulo 180 degrees */
    double cis[2], trans[2], o[2], a_mid[2], a_half[2], g_half[2], chi_tol[2];      /* (cos, sin) of the thresholds */
    double* out; long long out_stride;
    double* rows;                                   /* optional (B,Lab,8) */
    int* classes;                                   /* optional (B,Lab) */
    int gly, pro;                                   /* the residue types of phi_pos and cis_nonpro */
    int B, L, Lab;
} AbxTorsionArgs;
long long abx_torsion_scores_workspace_bytes(int B, int Lab);
int abx_torsion_scores(const AbxTorsionArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Secondary structure of designs: DSSP (Kabsch & Sander 1983) over the antibody rows - the electrostatic N-H...O=C energy between every
 * pair of residues on a virtual hydrogen, and from the bonds turns, helices, bridges, ladders and bends - against the crystal structure.
 * No upstream file:line: the reference has no such analysis (its evaluation is RMSD, AAR, cal_vio.py and PyRosetta); the definitions
 * are the ones written here.  One row of ABX_SECONDARY_COLS float64 values per structure of a batch of B designs of ONE complex
 * (abx_amd.secondary.SECONDARY_COLUMNS).  Declared limits: ALL bonds below the threshold are kept (mkdssp keeps the two best per
 * residue), no beta-bulge merging of ladders, no sheet labels, no kappa / alpha / phi / psi columns, I has the classic priority below G,
 * the antigen is not read, and the criterion is DSSP's electrostatic one, not the heavy-atom rule of abx_polar_scores.
 * The design and the complex are given as for abx_torsion_scores (pred_*, gt_*, res_mask, region, radius, chain_id, optional residx);
 * only the rows i < Lab are read.  All arithmetic is float64 from the float32 coordinates, no operation fused, sums as bracketed, sqrt
 * and / the IEEE ones.
 * PRESENT(i): N, CA, C and O (atom14 slots 0..3) of the row exist, and res_mask keeps it.
 * LINK (i-1, i), 1 <= i < Lab: chain_id equal, residx consecutive when given, both rows present.  CONT(i, j), i <= j: every link from
 *   i+1 to j holds.
 * DIST(a, b) = sqrt((dx*dx + dy*dy) + dz*dz), d = a - b.
 * H of row i: needs link (i-1, i) and a type other than `pro`;  v = C(i-1) - O(i-1);  n = sqrt((vx*vx + vy*vy) + vz*vz);
 *   H = N(i) + v / n component by component;  n == 0: the row has no H.
 * ENERGY of donor i (with an H) and acceptor j (present), j != i, and not j == i-1 with link (i-1, i):
 *   needs ((dx*dx + dy*dy) + dz*dz) < 81.0, d = CA_i - CA_j;
 *   e = 27.888 * (((1/DIST(N_i,O_j) + 1/DIST(H_i,C_j)) - 1/DIST(H_i,O_j)) - 1/DIST(N_i,C_j));  any of the four distances < 0.5: e = -9.9.
 *   hb(j -> i), C=O of j to N-H of i, holds when e < hb_energy (the caller's, finite and < 0; shipped -0.5 kcal/mol).
 * TURN_n(i), n = 3, 4, 5: CONT(i, i+n) and hb(i -> i+n).
 * BRIDGE(i, j): 1 <= i, j <= Lab-2, |i - j| >= 3, CONT(i-1, i+1) and CONT(j-1, j+1);
 *   parallel:      [hb(i-1 -> j) and hb(j -> i+1)] or [hb(j-1 -> i) and hb(i -> j+1)];
 *   antiparallel:  [hb(i -> j) and hb(j -> i)] or [hb(i-1 -> j+1) and hb(j-1 -> i+1)].   Both are symmetric in (i, j); chains may differ.
 * LADDERED: a parallel bridge (i, j) if (i+1, j+1) or (i-1, j-1) is a parallel bridge; an antiparallel one if (i+1, j-1) or (i-1, j+1)
 *   is an antiparallel bridge.
 * BEND(i): CONT(i-2, i+2);  u = CA_i - CA_(i-2);  v = CA_(i+2) - CA_i;  c = (ux*vx + uy*vy) + uz*vz;  the row bends when
 *   c < bend[0] * (|u| * |v|), |.| as DIST.  bend: (cos, sin) of 70 degrees, computed once on the host (abx_amd.secondary.thresholds)
 *   and checked as a unit pair.
 * STATE of row k, by order-free per-row rules; START_n(i) = TURN_n(i-1) and TURN_n(i):
 *   0 '.'  the row is not present;                      1 'H'  some i in [k-3, k] has START_4(i);
 *   4 'E' / 5 'B'  not H and the row has a bridge: E if one of its bridges is laddered, else B;
 *   2 'G'  not H, E, B and some i in [k-2, k] has START_3(i) with none of the rows i..i+2 being H, E or B;
 *   3 'I'  none of those and some i in [k-4, k] has START_5(i) with none of the rows i..i+4 being H, E, B or G;
 *   6 'T'  none of those and TURN_n(i) for some n and some i in [k-n+1, k-1];     7 'S'  none of those and BEND(k);     8 '-' otherwise.
 *   Three-state class: helix {H, G, I}, strand {E, B}, coil the rest.
 * A bond is an ordered (donor, acceptor) pair; "region end": its donor or its acceptor row is a region row.  A bridge pair is unordered
 * and counts once per type.
 *   0 n_hb             bonds in the antibody                  9-16 ss_H ss_G ss_I ss_E ss_B ss_T ss_S ss_C  region rows of the design by state
 *   1 n_hb_region      bonds with a region end               17 n_ss          region rows present in both structures
 *   2 n_hb_inside      bonds with both rows in the region    18 q8_same       ... with the same state in both
 *   3 hb_wild_region   the wild type's bonds of column 1     19 q3_same       ... with the same three-state class in both
 *   4 hb_kept_region   of those, the ones the design has     20 strand_ab     rows of the whole antibody in E or B
 *   5 hb_energy_region sum of e over the bonds of column 1   21 helix_ab      rows of the whole antibody in H, G or I
 *   6 n_bridge_region  bridge pairs with a region row         7 bridge_wild_region  the wild type's
 *   8 bridge_kept_region  bridge pairs in both structures, same pair and same type
 *   Column 5 is accumulated as rint(e * 2^20) in a 64-bit integer (the adds commute) and reported divided by 2^20.
 * rows: optional (B, Lab, 6) int32: the state, bonds donated, bonds accepted, the lowest and the next bridge partner row (-1: none), and
 * the flag word 1 region | 2 present | 4 has H | 8 parallel bridge | 16 antiparallel bridge | 32 bend | 64 / 128 / 256 TURN_3 / 4 / 5
 * starts here.  classes: optional (B, Lab) int32, the states.  out / out_stride as in AbxDesignScoreArgs (>= ABX_SECONDARY_COLS).
 * One launch, one workgroup of 256 per structure, the wild type first: N, CA, C, O staged as float32 in LDS (48 Lab bytes; widening at
 * the use is exact), one lane per donor with its own N and H in registers and the acceptor rows broadcast, the bonds of a donor as the
 * bits of its own row of an LDS matrix [Lab][ceil(Lab/32) | 1] written by that lane alone; then pattern phases of one lane per row
 * between barriers.  The wild type's bit image and one word per row (state, present, CONT(i-1, i+1)) go to this workgroup's slice of
 * the workspace and are read back, after a workgroup barrier, by the same workgroup.  Dynamic LDS up to 118400 bytes at Lab = 800, so
 * the entry raises the kernel's limit once per device; one workgroup per CU.  Lab <= ABX_SECONDARY_MAX_LAB; more is an argument error.
 * No allocation, no synchronisation.  The caller allocates the workspace (abx_secondary_scores_workspace_bytes). */
#define ABX_SECONDARY_COLS 22
#define ABX_SECONDARY_MAX_LAB 800
typedef struct AbxSecondaryArgs {
    const float* pred_atom14; long long pred_sb; int Lpred;
    const long long* pred_seq; long long pred_seq_sb;
    const unsigned char* pred_mask;                 /* optional (B,L,14) */
    const unsigned char* res_mask;                  /* optional (L) */
    const float* gt_atom14; const unsigned char* gt_exists; const long long* gt_seq;
    const unsigned char* region;                    /* optional (L) */
    const float* radius;                            /* [21][14] van-der-Waals radii as in AbxGuidanceArgs (> 0: the type has the slot) */
    const int* chain_id;                            /* (L) */
    const int* residx;                              /* optional (L) */
    double hb_energy;                               /* a bond: e < hb_energy; finite, < 0 */
    double bend[2];                                 /* (cos, sin) of the bend angle */
    double* out; long long out_stride;
    int* rows;                                      /* optional (B,Lab,6) */
    int* classes;                                   /* optional (B,Lab) */
    int pro;                                        /* the residue type without an H */
    int B, L, Lab;
} AbxSecondaryArgs;
long long abx_secondary_scores_workspace_bytes(int B, int Lab);
int abx_secondary_scores(const AbxSecondaryArgs* a, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Op-group entry points: one call per reference module of the pair stack, for a maintainer who binds
 * abx/model/seqformer.py without the Python orchestration of abx_amd/model/forward.py.  Each is a fixed sequence of the launches above
 * (abx_gemm descriptors filled here exactly as forward.py fills them; same kernels, same bits), asynchronous on the stream, no
 * allocation: weights come as packs built once by abx_pack_linear into caller memory, scratch as a caller workspace
 * (abx_*_workspace_bytes).  exact = 0: the split-f16 kernels (needs L >= 64 and B * L * L >= 32768 rows: what AbxGemm.exact = 2 serves);
 * exact = 1: the exact fp32-MFMA kernels (any size; triangle attention: L <= 389).  range_flag / range_tag: see AbxGemm.range_flag
 * (every launch of a group ORs the same tag).
 * ---------------------------------------------------------------------------------------------------------- */
/* One Linear (optionally with the preceding LayerNorm folded in), packed for both arithmetic paths.  All pointers point into the
 * caller's buffer handed to abx_pack_linear. */
typedef struct AbxLinearPack {
    const float* Wt;                    /* [K][N] fp32, rows scaled by the LayerNorm gamma when folded */
    const float* csum;                  /* [N] column sums of Wt (folded LayerNorm) or NULL */
    const float* bias;                  /* [N]: beta @ W^T + b (folded) / b / NULL */
    const unsigned short* planes;       /* abx_split_weights_f16 image [Kp/16][2][N][16] of Wt (of its k-permuted copy with ABX_PACK_PERMUTE_K16) */
    int b_exp;                          /* exponent of the planes */
    int K, N;
} AbxLinearPack;
/* a group of weight rows that becomes output columns: W [rows][K] (torch Linear.weight), b [rows] or NULL; glu: 0 = the sources
 * are concatenated in order; 1 / 2 = value / gate rows of a gated projection: channel c of the concatenated value (gate) sources
 * lands in column (c / 32) * 64 + c % 32 (+ 32), the (value, gate) column pairs of AbxGemm.glu */
typedef struct AbxLinearSrc { const float* W; const float* b; int rows; int glu; } AbxLinearSrc;
#define ABX_PACK_PERMUTE_K16 1          /* planes in the k order of the fused transition's second layer (0-3, 8-11, 4-7, 12-15 per 16) */
long long abx_pack_linear_bytes(int K, int N);
/* gamma / beta: [K] of the LayerNorm to fold, or NULL.  Synchronises the stream once (the plane exponent needs max |w| on the host):
 * packing is set-up work, outside any graph capture.  buf: 256-byte aligned device memory of abx_pack_linear_bytes(K, N). */
int abx_pack_linear(const AbxLinearSrc* src, int nsrc, int K, const float* gamma, const float* beta, int flags, void* buf,
                    AbxLinearPack* out, hipStream_t stream);

/* pair Transition (seqformer.py:358-376): z <- z + W2 relu(W1 LN(z) + b1) + b2 on rows [M][C], in place.
 * l1: pack of transition.1 with transition.0 (LayerNorm) folded; l2: pack of transition.3 with ABX_PACK_PERMUTE_K16.
 * exact = 0: ONE kernel (AbxGemm.mlp; C <= 192, no workspace); exact = 1: two GEMMs, workspace = M * l1.N floats. */
long long abx_transition_workspace_bytes(long long M, int hidden, int exact);
int abx_transition_fwd(const AbxLinearPack* l1, const AbxLinearPack* l2, float* z, long long M, int exact, void* workspace,
                       int* range_flag, int range_tag, hipStream_t stream);

/* TriangleMultiplication (seqformer.py:443-504), outgoing ('bikc,bjkc->bijc') or incoming ('bkic,bkjc->bijc').
 * glu: [left_proj | right_proj] (glu = 1) and [left_gate | right_gate] (glu = 2) with `norm` folded; out: proj_out with
 * `final_norm` folded; gate: final_gate with `norm` folded.  z_in (B, L*L, 192) -> z_out (B, L*L, 192), z_out != z_in (the tail
 * reads all channels of a row of z_in while other tiles write theirs); mask (B, L) float 0/1.  Split-f16 path only (exact = 0):
 * three launches - gated projections written as f16 operand images, plane x plane contraction, output projection * final gate +
 * residual.  The image region of the workspace must read zero where the kernels never write (pad k-tiles when ceil4(L) % 16 != 0):
 * abx_tri_mul_workspace_init once per (workspace, B, L). */
typedef struct AbxTriMulPack { AbxLinearPack glu, out, gate; } AbxTriMulPack;
long long abx_tri_mul_workspace_bytes(int B, int L);
int abx_tri_mul_workspace_init(void* workspace, int B, int L, hipStream_t stream);
int abx_tri_mul_fwd(const AbxTriMulPack* w, const float* z_in, float* z_out, const float* mask, int B, int L, int outgoing,
                    void* workspace, int* range_flag, int range_tag, hipStream_t stream);

/* TriangleAttention block (seqformer.py:506-550 + Attention.forward :272-312), starting node (per_row = 1) or ending node:
 * z <- z + proj_out(sigmoid(gate(LN z)) * attention(LN(z))) in place on (B, L*L, 192).  qkv: [proj_q | proj_k | proj_v] with `norm` folded;
 * gate: attn.gate with `norm` folded; pair: proj_pair (192 -> 4 heads) with `norm` folded; out: attn.proj_out packed with
 * ABX_PACK_PERMUTE_K16.  Launches (exact = 0): q | k | v GEMM with the pair bias in its grid (abx_gemm_side), bias transpose / pad (ending
 * node or L % 4 != 0), abx_tri_attn_fwd without a gate, then ONE gated tail (AbxGemm.mlp = 2): the gate projection, sigmoid, the product
 * with the attention output, the output projection and the residual - the gate never exists in memory.  With exact GEMMs the tail is two
 * launches (gate projection * attention output into the workspace, output projection + residual).  exact here is two bits: bit 0 the
 * GEMMs, bit 1 the attention kernel (a small complex runs exact GEMMs - too few rows for the split tiles - with the split-f16
 * attention, which has no size limit: exact = 1; everything exact: exact = 3). */
/* the head-major image of a q | k | v pack for abx_tri_attn_rowfused_fwd (AbxTriRowPack above).  qkv: LayerNorm-folded 192 -> 576 pack ([proj_q | proj_k | proj_v], 4 heads x 48 channels each) */
int abx_tri_rowpack(const AbxLinearPack* qkv, void* buf, AbxTriRowPack* out, hipStream_t stream);
/* row: optional (planes == NULL: never the row-fused route) - abx_tri_rowpack of qkv.  With it, exact = 0 and abx_tri_attn_rowfused_ok(L) the
 * launches are: the pair-bias projection alone (abx_gemm), the bias transpose / pad, abx_tri_attn_rowfused_fwd, the gated tail; the
 * q | k | v region of the workspace is not written.  Same bits as the route above. */
typedef struct AbxTriAttnPack { AbxLinearPack qkv, gate, pair, out; AbxTriRowPack row; } AbxTriAttnPack;
long long abx_tri_attn_block_workspace_bytes(int B, int L);
int abx_tri_attn_block_fwd(const AbxTriAttnPack* w, float* z, const float* mask, int B, int L, int per_row, int exact, void* workspace,
                           int* range_flag, int range_tag, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ABX_HIP_H */
