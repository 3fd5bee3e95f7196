// The main loop of the split-f16 tile kernels (gemm3.hip: the arithmetic, the operand layouts and the DMA pipeline are described there)
// and what goes with it: the counted wait + barrier of a k-step, the DMA sources of a plane image, the LayerNorm row statistics of a panel.
// Shared by the GEMM kernel families of gemm3.hip and the fused per-residue tails of tails.hip, which chain main loops on an A operand
// resident in LDS (AMODE 3).  Device only.
#pragma once
#include "common.h"
#include "abx_hip.h"
#include "split_dev.h"

constexpr int BK = 16;
#ifndef ABX_SPLIT_MIN_TILES
#define ABX_SPLIT_MIN_TILES 256     // smaller problems (sequence track, IPA) stay on the exact fp32 kernels
#endif

template <int N> __device__ __forceinline__ void wait_vm_and_barrier() {
    // own DMA writes for the next tile have landed (the newest N stay in flight), own LDS reads retired, then the block barrier
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// DMA source byte offsets (from the operand's batch base) of one wave for a [2][ROWS][16] 16-bit plane image stage: chunk c (1 KB of LDS) = wave * NL + i.
// Surplus chunks (image not a multiple of 4 KB) and rows past the matrix re-read a valid row; their LDS bytes are never used
// for valid outputs.
template <int ROWS, int NL, int NPL = 2>
__device__ __forceinline__ void plane_sources(long long s_plane, long long s_row, int r0, int R, unsigned (&off)[NL]) {
    // (the k-tile stride is applied by the caller: one k-tile = 16 consecutive k of every row)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        int o = (wave * NL + i) * 1024 + lane * 16;                 // byte offset in the stage
        if (o >= NPL * ROWS * 32) o -= NPL * ROWS * 32;             // surplus chunk: duplicate of the image start
        const int plane = o / (ROWS * 32), rem = o % (ROWS * 32);
        const int row = rem >> 5, hp = (rem >> 4) & 1;
        const int half = hp ^ ((row >> 3) & 1);
        const int gr = min(r0 + row, R - 1);
        off[i] = (unsigned)((plane * s_plane + (long long)gr * s_row + 8 * half) * 2);
    }
}

// Main loop of one output tile: acc += A' B for the operands of `g`; for the inline LayerNorm also the per-row partial sums
// (ls, lq over this lane's k half, shifted by lshift).  Ends with all DMA drained and a block barrier (the LDS is free again).
// SWAP: the MFMA operands trade places, acc[i][j] holds the TRANSPOSED 32 x 32 tile (rows = the tile's B rows / output columns, lane =
// A row): the fused transition consumes it as the A operand of its second GEMM straight from the registers.
// STATS: accumulate the inline LayerNorm partial sums and set lshift (the per-row shift of the operand, part of the statistics'
// meaning); a caller that walks the same A rows again passes STATS = false and the lshift of its first walk.
// AMODE 3: the A operand is resident in LDS (a_lds: BM fp32 rows of a_lds_stride bytes, k-contiguous; written by the caller before
// the call): no A stage, no A DMA - the fused IPA tail chains its GEMMs this way.
template <int BM, int BN, int WM, int WN, int AMODE, bool SWAP = false, bool STATS = true, int RING = 2>
__device__ __forceinline__ void gemm3_mainloop(const AbxGemm& g, float* smem, int mt, int nt, int b, f32x16 (&acc)[WM / 32][WN / 32],
                                               float (&ls)[WM / 32], float (&lq)[WM / 32], float (&lshift)[WM / 32],
                                               const char* a_lds = nullptr, int a_lds_stride = 0) {
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    constexpr int A_IMG = AMODE == 3 ? 0 : (AMODE == 2 ? 2 * BM * 32 : BM * 64);   // bytes per A stage (planes: the two pieces a0, a1)
    constexpr int NLA = AMODE == 3 ? 1 : (A_IMG + 4095) / 4096;                 // DMA instructions per wave per A tile
    constexpr int A_STAGE = RING == 2 ? A_IMG : (A_IMG + 4095) / 4096 * 4096;
    constexpr int B_IMG = 2 * BN * 32;
    constexpr int NLB = (B_IMG + 4095) / 4096;
    // with counted waits every wave must issue the same number of DMA instructions (stage padded to 4 KB multiples); the
    // 2-stage protocol waits for everything, so the surplus chunks are simply skipped and the stage is the bare image
    constexpr int B_STAGE = RING == 2 ? B_IMG : (B_IMG + 4095) / 4096 * 4096;   // (counted waits: the surplus chunks of a padded stage re-read the image start)
    // RING stages per operand: tile t + RING - 1 is fetched (DMA) while tile t is consumed.  RING = 2 (tile t + 1 waited for at the
    // end of step t) for the pair-stack GEMMs: with K <= 192 the fixed per-tile latencies (dispatch, first DMA, epilogue) weigh more
    // than pipeline depth, and the smaller LDS footprint buys a third / fourth resident block per CU (40 KB with 128x128 tiles, 52 KB
    // with 128x192) that hides them.  RING = 3 where ONE block owns the CU anyway (the IPA tail: 180 k-steps per block and nothing
    // else to hide a DMA round trip): two tiles in flight, counted waits (vmcnt: results return in issue order, so every wave must
    // issue the same NI instructions per tile - a stage is then padded to 4 KB and the surplus chunk loads rows nobody reads).
    constexpr int NI = (AMODE == 3 ? 0 : NLA) + NLB;
    constexpr int INFLIGHT = (RING - 2) * NI;                  // DMA instructions of this wave allowed to be outstanding at a wait

    char* As = reinterpret_cast<char*>(smem);                 // RING stages
    char* Bs = As + RING * A_STAGE;                           // RING stages
    const int m0 = mt * BM, n0 = nt * BN;
    // (the wave index as a scalar: the LDS destinations of the DMA instructions - m0 - are then SALU arithmetic, not a VALU
    // computation + v_readfirstlane per instruction)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int h = lane >> 5;

    // ---- DMA sources: a block-uniform base pointer (advanced per k-tile) plus per-lane 32-bit byte offsets, so the loads
    // use the scalar-base addressing form and cost no vector address arithmetic in the loop
    unsigned offsA[NLA], offsB[NLB];
    // The weight side first: its sources need two shifts, and with two stages its first k-tile is requested here, before the
    // integer divisions of the A-row maps below - a block's first DMA round trip is exposed (nothing of this block can run
    // before it lands), so it starts as early as the block knows where to read
    const char* baseB = reinterpret_cast<const char*>(
        g.B_split + ((g.batch_inner > 0 && g.A_split) ? (long long)(b / g.batch_inner) * g.sB3b + (long long)(b % g.batch_inner) * g.sB3i
                                                      : (long long)b * g.sB3b));
    plane_sources<BN, NLB>(g.sB3p, g.sB3n, n0, g.N, offsB);
    const long long b_step = g.sB3k * 2;
    const int nk = g.K / BK;
    auto issue_b = [&](int tile) {
        char* dst = Bs + (tile % RING) * B_STAGE + wave * NLB * 1024;
        const char* src = baseB + tile * b_step;
#pragma unroll
        for (int i = 0; i < NLB; ++i)
            if (RING > 2 || B_IMG % 4096 == 0 || (wave * NLB + i) * 1024 < B_IMG) glds16(src + vgpr32(offsB[i]), dst + i * 1024);
    };
    if constexpr (RING == 2) issue_b(0);
    const char* baseA = nullptr;
    long long a_step = 0;                                      // bytes per k-tile
    if constexpr (AMODE == 3) {
        offsA[0] = 0;
    } else if constexpr (AMODE == 0) {
        // offsets are relative to the tile's first row (to the batch base when the rows are pair-transposed)
        const bool remap = g.a_pair_transpose > 0 || g.a_pair != 0;
        const long long row0 = remap ? 0 : m0;
        baseA = reinterpret_cast<const char*>(g.A + (long long)b * g.sAb + row0 * g.sAm);
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int r = (wave * NLA + i) * 16 + (lane >> 2), p = lane & 3;
            const int kq = p ^ ((r >> 2) & 3);                 // physical 16-byte slot p of row r holds logical k-quad kq
            const long long gr = pair_a_row(g, min(m0 + r, g.M - 1));
            offsA[i] = (unsigned)(((gr - row0) * g.sAm + kq * 4) * 4);
        }
        a_step = BK * 4;
    } else if constexpr (AMODE == 1) {
        baseA = reinterpret_cast<const char*>(g.A + (long long)b * g.sAb + m0);
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            // LDS [k][BM]: a k-row is BM / 4 lanes of 16 bytes, so one instruction (64 lanes) brings 256 / BM k-rows: 2 of the 128-row
            // tile, 4 of the 64-row tile
            constexpr int LPR = BM / 4, KPI = 64 / LPR, LPR_LOG = BM == 128 ? 5 : 4;
            static_assert(LPR == 1 << LPR_LOG, "row-contiguous A: 128- or 64-row tiles");
            const int kl = (wave * NLA + i) * KPI + (lane >> LPR_LOG), mq = lane & (LPR - 1);
            const int gm = min(m0 + mq * 4, g.M - 4) - m0;                         // (M % 4 == 0: checked by the dispatch)
            offsA[i] = (unsigned)(((long long)kl * g.sAk + gm) * 4);
        }
        a_step = (long long)BK * g.sAk * 4;
    } else {
        baseA = reinterpret_cast<const char*>(g.A_split + (g.batch_inner > 0 ? (long long)(b / g.batch_inner) * g.sA3b + (long long)(b % g.batch_inner) * g.sA3i
                                                                                  : (long long)b * g.sA3b));
        plane_sources<BM, NLA>(g.sA3p, g.sA3m, m0, g.M, offsA);
        a_step = g.sA3k * 2;
    }

    auto issue_a = [&](int tile) {          // tile index clamped by the caller
        if constexpr (AMODE == 3) return;
        char* dst = As + (tile % RING) * A_STAGE + wave * NLA * 1024;
        const char* src = baseA + tile * a_step;
#pragma unroll
        for (int i = 0; i < NLA; ++i)
            if (RING > 2 || A_IMG % 4096 == 0 || (wave * NLA + i) * 1024 < A_IMG) glds16(src + vgpr32(offsA[i]), dst + i * 1024);
    };

#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float m2048 = -2048.0f;
    asm volatile("" : "+v"(m2048));                           // (a VGPR constant of split2h_mix; not rematerialised into an SGPR)
    const bool relu = g.a_relu != 0;
    const bool ln_inline = g.ln_csum != nullptr && g.ln_stats == nullptr;
    f32x2 ls2[TM], lq2[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        ls[i] = lq[i] = 0.f;
        if constexpr (STATS) lshift[i] = 0.f;
        ls2[i] = lq2[i] = (f32x2){0.f, 0.f};
    }

    // prologue
#pragma unroll
    for (int r = 0; r < RING - 1; ++r) {
        issue_a(min(r, nk - 1));
        if constexpr (RING != 2) issue_b(min(r, nk - 1));
    }
    wait_vm_and_barrier<INFLIGHT>();

    // per-lane LDS fragment offsets
    int offA[TM][(AMODE == 0 || AMODE == 3) ? 2 : 1];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = wm * WM + i * 32 + (lane & 31);
        if constexpr (AMODE == 3) {
            offA[i][0] = r * a_lds_stride + (2 * h) * 16;
            offA[i][1] = r * a_lds_stride + (2 * h + 1) * 16;
        } else if constexpr (AMODE == 0) {
            const int x = (r >> 2) & 3;
            offA[i][0] = r * 64 + (((2 * h) ^ x) << 4);
            offA[i][1] = r * 64 + (((2 * h + 1) ^ x) << 4);
        } else if constexpr (AMODE == 1) {
            offA[i][0] = (8 * h) * (BM * 4) + r * 4;
        } else {
            offA[i][0] = plane_off<BM>(0, r, h);
        }
    }
    int offB[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) offB[j] = plane_off<BN>(0, wn * WN + j * 32 + (lane & 31), h);

    // a wave whose 32 rows all lie beyond M (the last row tile of a ragged M: e.g. the 4th wave of the third 128-row tile of the
    // L = 352 contraction) takes part in the DMA and the barriers but skips its B-fragment reads and MFMAs
    const bool rows_live = m0 + wm * WM < g.M;
    if (!rows_live) {
        for (int t = 0; t < nk; ++t) {
            issue_b(min(t + RING - 1, nk - 1));
            issue_a(min(t + RING - 1, nk - 1));
            wait_vm_and_barrier<INFLIGHT>();
        }
    } else
    for (int t = 0; t < nk; ++t) {
        // next tiles
        issue_b(min(t + RING - 1, nk - 1));
        issue_a(min(t + RING - 1, nk - 1));
        const char* as = AMODE == 3 ? a_lds + t * 64 : As + (t % RING) * A_STAGE;
        const char* bs = Bs + (t % RING) * B_STAGE;
        u32x4 a[TM][2];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            if constexpr (AMODE == 2) {
#pragma unroll
                for (int p = 0; p < 2; ++p) a[i][p] = *reinterpret_cast<const u32x4*>(as + offA[i][0] + p * (BM * 32));
            } else {
                float x[8];
                if constexpr (AMODE == 0 || AMODE == 3) {
                    const f32x4 lo = *reinterpret_cast<const f32x4*>(as + offA[i][0]);
                    const f32x4 hi = *reinterpret_cast<const f32x4*>(as + offA[i][1]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) { x[c] = lo[c]; x[4 + c] = hi[c]; }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) x[e] = *reinterpret_cast<const float*>(as + offA[i][0] + e * (BM * 4));
                }
                if (ln_inline) {
                    // statistics of the row from this lane's 8 k (the other k half sits in lane ^ 32), shifted by the row's
                    // first element so that E[x^2] - mean^2 does not cancel when |mean| >> sigma.  Packed math: two elements
                    // per VALU instruction (even / odd partial sums, folded after the loop)
                    if (STATS && t == 0) lshift[i] = __shfl(x[0], lane & 31, 64);
                    const f32x2 sh2 = {lshift[i], lshift[i]};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        f32x2 xp = {x[2 * e], x[2 * e + 1]};
                        xp -= sh2;
                        if constexpr (STATS) {
                            ls2[i] += xp;
                            lq2[i] = __builtin_elementwise_fma(xp, xp, lq2[i]);
                        }
                        x[2 * e] = xp[0];
                        x[2 * e + 1] = xp[1];
                    }
                }
                if (relu) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) x[e] = fmaxf(x[e], 0.f);
                }
                unsigned q0[4], q1[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    split2h_mix(x[2 * e], x[2 * e + 1], m2048, q0[e], q1[e]);
                }
                a[i][0] = u32x4{q0[0], q0[1], q0[2], q0[3]};
                a[i][1] = u32x4{q1[0], q1[1], q1[2], q1[3]};
            }
        }
        // product terms, smallest first (SplitTerms); the B fragments are fetched per group of JG sub-tiles (register budget);
        // consecutive MFMAs hit different accumulators
        using T = SplitTerms;
        constexpr int JG = TN > 3 ? (TN % 3 == 0 ? 3 : 2) : TN;
#pragma unroll
        for (int j0 = 0; j0 < TN; j0 += JG) {
            u32x4 bb[JG][3];
#pragma unroll
            for (int j = 0; j < JG; ++j)
#pragma unroll
                for (int p = 0; p < 2; ++p) bb[j][p] = *reinterpret_cast<const u32x4*>(bs + offB[j0 + j] + p * (BN * 32));
#pragma unroll
            for (int j = 0; j < JG; ++j) bb[j][2] = f16x8_lo(bb[j][0]);
#pragma unroll
            for (int term = 0; term < T::N; ++term)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < JG; ++j)
                        acc[i][j0 + j] = SWAP ? mfma_split(bb[j][T::B[term]], a[i][T::A[term]], acc[i][j0 + j])
                                              : mfma_split(a[i][T::A[term]], bb[j][T::B[term]], acc[i][j0 + j]);
        }
        wait_vm_and_barrier<INFLIGHT>();
    }
    if constexpr (AMODE != 2) {
        // the planes hold w * 2^b_exp, the activations went in as x * 2^ABX_F16_A_EXP: exact power-of-two rescale
        // (plane x plane: the images were written as x 2^-4 and y 2^4, nothing to undo)
        const float cs = __builtin_ldexpf(1.0f, -ABX_F16_A_EXP - g.b_exp);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] *= cs;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        ls[i] = ls2[i][0] + ls2[i][1];
        lq[i] = lq2[i][0] + lq2[i][1];
    }
    // drain the (redundant) tail DMA before the epilogue reuses the LDS
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
}

// LayerNorm row statistics of this M-panel -> st_lds [BM][2] (mean - shift, rstd); returns whether the GEMM is LN-folded
template <int BM, int BN, int WM, int WN, bool EDGE>
__device__ __forceinline__ bool gemm3_row_stats(const AbxGemm& g, float* st_lds, int mt, int b, const float (&ls)[WM / 32],
                                                const float (&lq)[WM / 32]) {
    constexpr int TM = WM / 32, WAVES_N = BN / WN;
    const int m0 = mt * BM;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N, h = lane >> 5;
    const bool ln_inline = g.ln_csum != nullptr && g.ln_stats == nullptr;
    const float* gstats = g.ln_stats ? g.ln_stats + 2 * (long long)b * g.sSb : nullptr;
    if (gstats) {
        for (int idx = threadIdx.x; idx < 2 * BM; idx += 256) {
            const int m = m0 + (idx >> 1);
            st_lds[idx] = (!EDGE || m < g.M) ? gstats[2 * (long long)m + (idx & 1)] : 0.f;
        }
    } else if (ln_inline) {
        const float invK = 1.0f / (float)g.K;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float sm = ls[i] + __shfl_xor(ls[i], 32, 64), sq = lq[i] + __shfl_xor(lq[i], 32, 64);
            if (wn == 0 && h == 0) {                            // the wn waves hold identical copies
                const int row = wm * WM + i * 32 + lane;
                const float dm = sm * invK;
                st_lds[2 * row] = dm;                           // the operand was shifted: only (mean - shift) remains
                st_lds[2 * row + 1] = 1.0f / sqrtf(fmaxf(sq * invK - dm * dm, 0.f) + g.ln_eps);
            }
        }
    }
    return gstats != nullptr || ln_inline;
}
