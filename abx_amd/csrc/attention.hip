// Pair-biased softmax attention kernels of the Seqformer block.
//
// abx_tri_attn_fwd — triangle attention (reference abx/model/seqformer.py:506-550, Attention.forward :272-312) as a
// flash-style fused kernel: the (B, L, 4, L, L) logits tensor (268 MB / sample at L = 256) is never materialised.
// One workgroup per (b, row s, head h): K [L][48] and V [L][48] of that row are staged ONCE in LDS (row stride 52 floats;
// K rows permuted so a lane's 12 QK^T operands are three 16-byte reads); each of the 12 waves (3 per SIMD, so one wave's softmax VALU / LDS
// latency hides under the others' MFMAs) walks query tiles of 16 rows with a base-2 online softmax over 64-key tiles; the pair bias of
// a tile is fetched before its QK^T MFMAs.  Both contractions run on v_mfma_f32_16x16x4_f32 (exact fp32):
//     S^T[key][q]  = sum_d K[key][d] * Q[q][d]        ("swapped" QK^T: a lane owns 4 keys of ONE query column, so the
//                                                      softmax row reductions are in-lane + two cross-group shuffles)
//     O^T[d][q]   += sum_key V[key][d] * P[key][q]    (P fragments feed the B operand straight from registers)
// The orientation (starting / ending node) is expressed only through strides; no transposed copy of the pair stack.
//
// abx_tri_attn_rowfused_fwd — the same attention for rows of L <= 352 with the q | k | v projection of the row inside the kernel
// (tri_attn8_rowfused_kernel below: phase P projects [k | v | q] of the row's head from LayerNorm(z[b, s]) with the arithmetic of the
// split-f16 GEMM straight into the K / V planes in LDS and the Q fragments in registers, phase A is the computing-wave body of tri_attn8):
// q | k | v never travel through HBM; bit-identical to the projection GEMM followed by abx_tri_attn_fwd.
//
// abx_seq_attn_fwd — sequence attention with 32-head pair bias (seqformer.py:314-356, split_first=False :278-281):
// lanes are keys so that the bias rows are read coalesced, K/V of the (b, h) pair in LDS.
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "common.h"
#include "abx_hip.h"
#include "split_dev.h"
#include "tri_row_touch.h"

namespace {

constexpr int TD = 48;        // head dim of triangle attention
constexpr int LDK = 52;       // K rows are stored permuted [key][g][kd] (d = kd*4 + g): a lane's 12 operands are 3 x 16-byte reads
constexpr int LDV = 52;       // V row stride: 4*52 mod 32 == 16 -> lane groups g land on disjoint bank halves

constexpr int TRI_THREADS = 768;      // 12 waves = 3 per SIMD: softmax VALU / LDS latency of one wave hide under the others' MFMAs
constexpr float LOG2E = 1.4426950408889634f;

// KC: keys per staged chunk (== L: the whole row once, the round-1 form; otherwise a multiple of 64).  A row longer than the LDS holds (L > 389) is
// walked in key chunks: the 12 waves take 12 query tiles at a time through ALL chunks (online softmax across chunks, state in
// registers), re-staging the chunks for every group of 12 query tiles - the exact kernel is the fallback of the split-f16 one, the
// re-reads are the price of having no length limit (seqformer.py:272-312 has none).
__global__ __launch_bounds__(TRI_THREADS) void tri_attn_kernel(const AbxTriAttn a, const int KC) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L = a.L;
    float* Ks = smem;
    float* Vs = smem + (((size_t)KC * LDK + 3) & ~(size_t)3);     // keep V rows 16-byte aligned
    float* Ms = Vs + (size_t)KC * LDV;                            // [KC + 1]: key classes of the chunk's slots, [KC] = any key masked
    const int h = blockIdx.x, s = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 15, g = lane >> 4;
    const int nchunk = (L + KC - 1) / KC;

    const long long base = (long long)b * a.sb + (long long)s * a.ss + (long long)h * TD;
    const float* km = a.keymask ? a.keymask + (long long)b * a.km_sb : nullptr;
    // does the sample mask any key?  (decides the clamp-free path, as a whole-row property like before)
    // (through a slot of the dynamic LDS: __syncthreads_or would add static LDS, and the kernel asks for all 160 KB dynamically)
    float* flag = Ms + ((KC + 63) / 64) * 64;
    if (tid == 0) *flag = 0.f;
    __syncthreads();
    if (km) {
        bool any_masked = false;
        for (int key = tid; key < L; key += TRI_THREADS) any_masked |= km[key] == 0.f;
        if (any_masked) *flag = 1.f;                             // benign race: every writer stores the same value
    }
    __syncthreads();
    const bool has_mask = *flag != 0.f;
    // ---- stage K, V and the key classes of chunk c: 0 (valid), 1 (masked: the reference REPLACES the logit by finfo.min), 2 (beyond L)
    auto stage = [&](int c) {
        const int c0 = c * KC, nk = min(KC, L - c0);
        for (int idx = tid; idx < nk * (TD / 4); idx += TRI_THREADS) {
            const int key = idx / (TD / 4), c4 = idx % (TD / 4);
            const long long off = base + (long long)(c0 + key) * a.sl + c4 * 4;
            const f32x4 kv = *reinterpret_cast<const f32x4*>(a.k + off);
            const f32x4 vv = *reinterpret_cast<const f32x4*>(a.v + off);
            float* kd = Ks + key * LDK + c4;                     // element d = c4*4 + j goes to [g = j][kd = c4]
            kd[0] = kv[0]; kd[12] = kv[1]; kd[24] = kv[2]; kd[36] = kv[3];
            *reinterpret_cast<f32x4*>(Vs + key * LDV + c4 * 4) = vv;
        }
        const int npad = ((nk + 63) / 64) * 64;
        for (int key = tid; key < npad; key += TRI_THREADS)
            Ms[key] = key < nk ? ((!km || km[c0 + key] != 0.f) ? 0.f : 1.f) : 2.f;
    };
    if (nchunk == 1) {
        stage(0);
        __syncthreads();
    }

    const float* biasb = a.bias ? a.bias + (long long)b * a.bias_sb + (long long)h * a.bias_sh : nullptr;
    const int nqt = (L + 15) / 16;
    const bool bias_vec = biasb && a.bias_sk == 1 && (a.bias_sq % 4 == 0) && (L % 4 == 0) &&
                          ((reinterpret_cast<uintptr_t>(biasb) & 15) == 0);
    const float qscale = a.scale * LOG2E;                       // softmax evaluated in base 2: exp(x) = exp2(x log2 e)
    const float bias_l2 = a.bias_log2 ? 0.0078125f : LOG2E;     // (a bias that arrives as ABX_TRI_BIAS_LOG2 x the pair bias: back to base-2 logits)

    for (int qg = 0; qg < nqt; qg += TRI_THREADS / 64) {
        const int qt = qg + wave;
        const bool has_tile = qt < nqt;                          // (a wave without a tile still joins the chunk barriers)
        // ---- Q fragment (B operand of the swapped product): lane holds Q[q][kd*4 + g], pre-scaled
        const int qrow = qt * 16 + lq;
        const bool qok = has_tile && qrow < L;
        float qf[12];
        {
            const float* qp = a.q + base + (long long)(qok ? qrow : 0) * a.sl + g;
#pragma unroll
            for (int kd = 0; kd < 12; ++kd) qf[kd] = qok ? qp[kd * 4] * qscale : 0.f;
        }
        const float* brow = biasb ? biasb + (long long)(qok ? qrow : 0) * a.bias_sq : nullptr;
        float m_run = -INFINITY, l_run = 0.f;
        f32x4 o[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};

        // one 64-key tile of the staged chunk (first key c0, nk keys).  FAST: the tile lies fully inside the chunk and no key is masked
        // -> no clamps, no mask arithmetic, LDS addresses are a per-tile base plus compile-time offsets.
        auto tile = [&](const int c0, const int nk, const int kt, auto fast_tag) {
            constexpr bool FAST = decltype(fast_tag)::value;
            const int k0 = kt * 64;                               // chunk-local
            // ---- bias of this tile: issued first so the loads fly under the QK^T MFMAs
            float bz[4][4];
            if (bias_vec && (FAST || k0 + 64 <= nk)) {           // 4 consecutive keys per lane -> one 16-B load (c0 % 64 == 0)
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(brow + c0 + k0 + sub * 16 + g * 4);
                    bz[sub][0] = t4[0]; bz[sub][1] = t4[1]; bz[sub][2] = t4[2]; bz[sub][3] = t4[3];
                }
            } else {
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = FAST ? k0 + sub * 16 + g * 4 + r : min(k0 + sub * 16 + g * 4 + r, nk - 1);
                        bz[sub][r] = brow ? brow[(long long)(c0 + key) * a.bias_sk] : 0.f;
                    }
            }
            f32x4 sc[4];
            // ---- S^T tiles: 4 sub-blocks of 16 keys
            const float* kbase = Ks + (k0 + lq) * LDK + g * 12;
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) {
                const f32x4* kp = reinterpret_cast<const f32x4*>(
                    FAST ? kbase + sub * 16 * LDK : Ks + min(k0 + sub * 16 + lq, nk - 1) * LDK + g * 12);
                const f32x4 ka = kp[0], kb4 = kp[1], kc = kp[2];
                f32x4 c0a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kd = 0; kd < 4; ++kd) c0a = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[kd], qf[kd], c0a, 0, 0, 0);
#pragma unroll
                for (int kd = 0; kd < 4; ++kd) c0a = __builtin_amdgcn_mfma_f32_16x16x4f32(kb4[kd], qf[4 + kd], c0a, 0, 0, 0);
#pragma unroll
                for (int kd = 0; kd < 4; ++kd) c0a = __builtin_amdgcn_mfma_f32_16x16x4f32(kc[kd], qf[8 + kd], c0a, 0, 0, 0);
                sc[sub] = c0a;
            }
            // this lane: keys k0 + sub*16 + g*4 + r (r = 0..3) of query column lq
            float mx = -INFINITY;
            if (FAST) {
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = fmaf(bz[sub][r], bias_l2, sc[sub][r]);
                        sc[sub][r] = v;
                        mx = fmaxf(mx, v);
                    }
            } else {
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    const f32x4 mk = *reinterpret_cast<const f32x4*>(Ms + k0 + sub * 16 + g * 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = fmaf(bz[sub][r], bias_l2, sc[sub][r]);
                        v = mk[r] == 0.f ? v : (mk[r] == 1.f ? ABX_NEG_MAX : -INFINITY);
                        sc[sub][r] = v;
                        mx = fmaxf(mx, v);
                    }
                }
            }
            // ---- online softmax update of this query column
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // m_run = -inf on the first tile -> 0
            float rs = 0.f;
#pragma unroll
            for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(sc[sub][r] - m_new);   // arguments <= 0: raw v_exp_f32
                    sc[sub][r] = p;
                    rs += p;
                }
            rs += __shfl_xor(rs, 16, 64);
            rs += __shfl_xor(rs, 32, 64);
            l_run = l_run * alpha + rs;
            m_run = m_new;
            if (!__all(alpha == 1.0f)) {                        // the running maximum rarely moves after the first tiles
#pragma unroll
                for (int d = 0; d < 3; ++d)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[d][r] *= alpha;
            }
            // ---- O^T += V^T P : MFMA step (sub, r) contracts keys {k0 + sub*16 + g*4 + r : g = 0..3}
            const float* vbase = Vs + (k0 + g * 4) * LDV + lq;
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* vp = FAST ? vbase + (sub * 16 + r) * LDV
                                           : Vs + min(k0 + sub * 16 + g * 4 + r, nk - 1) * LDV + lq;   // p == 0 for keys beyond the row
#pragma unroll
                    for (int d = 0; d < 3; ++d)
                        o[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[d * 16], sc[sub][r], o[d], 0, 0, 0);
                }
            }
        };
        for (int c = 0; c < nchunk; ++c) {
            const int c0 = c * KC, nk = min(KC, L - c0);
            if (nchunk > 1) {
                __syncthreads();                                // every wave has left the chunk staged before
                stage(c);
                __syncthreads();
            }
            if (has_tile) {
                const int nkt = (nk + 63) / 64, nfast = has_mask ? 0 : nk / 64;
                for (int kt = 0; kt < nfast; ++kt) tile(c0, nk, kt, std::true_type{});
                for (int kt = nfast; kt < nkt; ++kt) tile(c0, nk, kt, std::false_type{});
            }
        }
        // ---- normalise, gate, store.  O^T layout: column = query lq, rows d = dblk*16 + g*4 + r
        if (qok) {
            const float inv = 1.0f / l_run;
            const long long go = base + (long long)qrow * a.sl;
            float* op = a.out + (long long)b * a.ob + (long long)s * a.os + (long long)qrow * a.ol + h * TD;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int dd = d * 16 + g * 4;
                f32x4 v = o[d];
                if (a.gate) {
                    const f32x4 gv = *reinterpret_cast<const f32x4*>(a.gate + go + dd);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = v[r] * inv * sigmoidf_(gv[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] *= inv;
                }
                *reinterpret_cast<f32x4*>(op + dd) = v;
            }
        }
    }
}

// ---- triangle attention on the float16 matrix cores (split-f16, see gemm3.hip for the arithmetic) ----------------------------
// Same (b, row s, head h) decomposition, online softmax and swapped S^T product as tri_attn_kernel, with every fp32 product evaluated
// from 3 exact f16 products (v_mfma_f32_16x16x32_f16, fp32 accumulate): keys / values are the plane side (16 k, 16 v as p0, p1,
// p2 = p0 2^-11), queries and softmax weights the two-piece side (q / 16, P / 16 as a0, a1), so the products need no rescale.
//   K, V of the row are split ONCE, while they are staged, in chunks of 192 / 128 keys (p0, p1; p2 = p0 2^-11 is derived at the
//   fragment: two planes per operand leave room for 192-key chunks, i.e. two chunks and two barriers at L = 352), DOUBLE BUFFERED: the global loads of chunk
//   c + 1 are issued before the wave computes on chunk c and are split + written afterwards, ONE barrier per chunk.
//     K planes [2][key][48 d] f16 (96-byte rows)   -> A operand of S^T = K Q^T          (lane: key, 8 consecutive d; ds_read_b128)
//     V planes [2][key][48 d] f16 (same image)     -> A operand of O^T += V^T P         (lane: d, 8 keys) through the transposing
//                                                     LDS read ds_read_b64_tr_b16: a 16-lane group reads a [4 keys][16 d] block
//                                                     and lane n receives its column n; no transposed staging writes
//   Q is split per query tile in registers; P per key tile in registers: the S^T accumulators of two 16-key sub-blocks (lane:
//   query lq, keys 4g + r) are exactly the 8 k-values lane (m = lq, k-group g) feeds to the A operand of one PV MFMA.
//   O^T[d][q] accumulators: column = query like the S^T tiles, so the running (max, sum) and the rescale are lane-local; the
//   four-lane reductions of a query column use v_permlane16/32_swap (VALU), never the LDS queue.
//   The pair bias is read in rows of bias_sq floats (bias_sk == 1: rows padded to a multiple of 4 -> 16-byte loads for any L).
//   Grid: 1-D, ordered so that the workgroups resident on one XCD walk the rows of ONE (b, h) pair: its (L, L) bias (495 KB at
//   L = 352) stays in that XCD's L2 instead of being re-fetched from HBM by every row.
constexpr int RST = 96;                  // bytes per key row of a plane: 32 * odd -> 16-byte fragment reads of 16 consecutive rows hit 64 banks

// two-piece split of a pre-scaled pair without the 2^11 lift of the remainder (tri_attn8_kernel: operands scaled so that it stays a
// normal float16 where it matters): x = p0 + p1 (+ <= 2^-24 |x|, or 2^-25 absolute below |x| = 2^-2)
__device__ __forceinline__ void split2h_ns(float a, float b, unsigned& p0, unsigned& p1) {
    // p0 = (f16(a), f16(b)); p1 = (f16(a - p0.lo), f16(b - p0.hi)): the differences are exact in fp32, so the mixed-precision FMA
    // (f16 source, f32 addend, f16 result: one rounding) gives the bits of convert - subtract - convert in 3 instructions instead of 5
    p0 = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, f16x2));
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(p1) : "v"(p0), "v"(a));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(p1) : "v"(p0), "v"(b));
}

// common.h split2b (planes p0 = f16(16 x), p1 = f16(16 x - p0)) on the mixed-precision FMA: 16 x - p0 is exact in fp32, so one
// rounding to f16 gives the bits of scale - convert - convert back - subtract - convert, in 4 instructions per pair instead of 6
// (the producer wave of tri_attn8_kernel is what the chunk barrier waits for).  c16 = 16.0f in a VGPR (no literal in VOP3P).
__device__ __forceinline__ void split2b_mix(float a, float b, float c16, unsigned& p0, unsigned& p1) {
    asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "=v"(p0) : "v"(a), "v"(c16));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "+v"(p0) : "v"(b), "v"(c16));
    asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(p1) : "v"(a), "v"(c16), "v"(p0));
    asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(p1) : "v"(b), "v"(c16), "v"(p0));
}

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// single-instruction max / min (the compiler otherwise canonicalises MFMA results with an extra v_max before fmaxf / fminf)
__device__ __forceinline__ float vmax(float x, float y) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
__device__ __forceinline__ float vmin(float x, float y) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}

__device__ __forceinline__ float vmax3(float x, float y, float z) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
    return r;
}
// Reductions over the four lanes {l, l^16, l^32, l^48} (one query column of the swapped S^T tiles) on the VALU path:
// v_permlane16_swap / v_permlane32_swap exchange 16- / 32-lane halves in a few cycles, where __shfl_xor goes through the LDS
// queue (ds_bpermute) behind the K / V fragment reads of all 12 waves - four serial LDS round trips per key tile were the
// largest single cost of this kernel.
__device__ __forceinline__ float quad_max(float x) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = vmax(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return vmax(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float quad_sum(float x) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

__device__ __forceinline__ s16x4 lds_tr16(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

// KC4: keys per chunk; DB: double-buffered chunks (next chunk's loads ride under this chunk's compute, one barrier per chunk) or
// a single buffer (load -> split -> write between two barriers at every chunk start, but fewer, larger chunks)
template <int MAXQ, int KC4, bool DB, int NTH, bool PROD>
__global__ __launch_bounds__(NTH) void tri_attn4_kernel(const AbxTriAttn a) {
    constexpr int PLN = KC4 * RST;           // bytes per plane
    constexpr int BUF4 = 4 * PLN;            // K planes + V planes (p0, p1 each; p2 = p0 2^-11 is derived at the fragment) of one chunk
    constexpr int NIT = (KC4 * (TD / 4) + NTH - 1) / NTH;     // staging items per thread and chunk
    // PROD: the last wave is a PRODUCER - it alone stages the next chunk (loads, splits, LDS writes) while the other NCW waves
    // compute.  Vector-memory results return in issue order, so a consumer that also carried staging loads (HBM latency) waited for
    // them at its next bias use (L2 latency); with L = 352 the 22 query tiles are exactly 2 slots of 11 consumer waves.
    constexpr int NCW = NTH / 64 - (PROD ? 1 : 0);
    static_assert(!PROD || DB, "producer wave: double-buffered chunks");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* lds = reinterpret_cast<char*>(smem);
    float* Msb = reinterpret_cast<float*>(lds + (DB ? 2 : 1) * BUF4);       // [2][KC4] key-mask clamps of the chunks in flight
    const int L = a.L;
    // ---- (b, h, s) of this workgroup: XCD x (blockIdx & 7) owns the (b, h) pairs x, x + 8, ... and walks their rows in order
    // Long rows: the query tiles of a row are dealt to q_parts workgroups (each stages all keys of the row; neighbours in the grid, so
    // the row's K / V come from the L2 the second time): a wave never carries more than MAXQ tiles of online-softmax state.
    // When B * H is not a multiple of 8 (one sample: 4 pairs - half of the XCDs would idle) the rows of every pair are dealt to
    // row_groups = 2 virtual pairs (even / odd rows), which always gives a multiple of 8 with H = 4.
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int G = a.row_groups, rows_g = (a.S + G - 1) / G;
    const int per_vp = rows_g * a.q_parts, sp = slot % per_vp;
    const int vp = (slot / per_vp) * 8 + xcd;
    const int bh = vp / G, s = (sp / a.q_parts) * G + vp % G, part = sp % a.q_parts;
    if (bh >= a.B * a.H || s >= a.S) return;
    const ClockProbe probe(a.clock_probe);
    const int b = bh / a.H, h = bh % a.H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 15, g = lane >> 4;
    const long long base = (long long)b * a.sb + (long long)s * a.ss + (long long)h * TD;
    const float* km = a.keymask ? a.keymask + (long long)b * a.km_sb : nullptr;
    const float* biasb = a.bias ? a.bias + (long long)b * a.bias_sb + (long long)h * a.bias_sh : nullptr;
    const int nqt_row = (L + 15) / 16, tpp = (nqt_row + a.q_parts - 1) / a.q_parts;   // query tiles of the row / of one part
    const int qt0 = part * tpp, nqt = min(nqt_row, qt0 + tpp);
    const bool bias_vec = biasb && a.bias_sk == 1 && (a.bias_sq % 4 == 0) && ((reinterpret_cast<uintptr_t>(biasb) & 15) == 0);
    const int bias_row = (int)a.bias_sq;                        // readable floats per bias row when bias_sk == 1
    // split-f16 scales: keys / values are staged as 16 x, queries and softmax weights enter as x / 16, so the products need no rescale
    const float qscale = a.scale * LOG2E * 0.0625f;
    const float bias_l2 = a.bias_log2 ? 0.0078125f : LOG2E;     // (see tri_attn_kernel)
    // wave-uniform: does this sample mask any key?  (12 waves x 64 lanes cover L <= 768 in one pass of the ballot loop)
    bool any_masked = false;
    if (km) {
        for (int j = lane; j < L; j += 64) any_masked |= km[j] == 0.f;
        any_masked = __any(any_masked);
    }

    float m_run[MAXQ], l_run[MAXQ];
    f32x4 o[MAXQ][3];
#pragma unroll
    for (int sl = 0; sl < MAXQ; ++sl) {
        m_run[sl] = -INFINITY;
        l_run[sl] = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) o[sl][d] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    // staging share of this thread: 2 (key, 4-channel) items of a chunk: 128 keys x 12 float4 = 1536 items over 768 threads.
    // Item `it` of the NEXT chunk is loaded before and written after the wave's query-tile slot `it` of the current chunk (the
    // other buffer was last read before the previous barrier), so only one item is live in registers at a time.
    f32x4 kreg, vreg;
    auto stage_load = [&](int c0, int idx) {
        const int kk = idx / (TD / 4), c4 = idx % (TD / 4);
        kreg = (f32x4){0.f, 0.f, 0.f, 0.f};
        vreg = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (kk < KC4 && c0 + kk < L) {
            const long long off = base + (long long)(c0 + kk) * a.sl + c4 * 4;
            // read once per launch: non-temporal, so that the K / V stream does not push the Q rows (re-read at every chunk) and the
            // pair's bias out of the L2
            kreg = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.k + off));
            vreg = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.v + off));
        }
    };
    auto stage_mask = [&](int c0, int buf, int t) {
        Msb[buf * KC4 + t] = (c0 + t < L) ? ((!km || km[c0 + t] != 0.f) ? INFINITY : ABX_NEG_MAX) : -INFINITY;
    };
    auto stage_write = [&](int c0, int buf, int idx) {
        char* Kp = lds + buf * BUF4;
        char* Vp = Kp + 2 * PLN;
        const int kk = idx / (TD / 4), c4 = idx % (TD / 4);
        if (kk >= KC4) return;
        unsigned a0, a1, b0, b1;
        split2b(kreg[0], kreg[1], a0, a1);
        split2b(kreg[2], kreg[3], b0, b1);
        char* kd = Kp + kk * RST + c4 * 8;
        *reinterpret_cast<u32x2*>(kd) = u32x2{a0, b0};
        *reinterpret_cast<u32x2*>(kd + PLN) = u32x2{a1, b1};
        split2b(vreg[0], vreg[1], a0, a1);
        split2b(vreg[2], vreg[3], b0, b1);
        char* vd = Vp + kk * RST + c4 * 8;
        *reinterpret_cast<u32x2*>(vd) = u32x2{a0, b0};
        *reinterpret_cast<u32x2*>(vd + PLN) = u32x2{a1, b1};
    };
    // (key-mask clamps are applied as logit = min(logit, clamp): +inf valid, finfo.min masked (the reference REPLACES the logit by
    // finfo.min: every finite logit is >= finfo.min, so min() is that replacement), -inf beyond L)

    if (DB) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) { stage_load(0, tid + it * NTH); stage_write(0, 0, tid + it * NTH); }
        if (tid < KC4) stage_mask(0, 0, tid);
        __syncthreads();
    }

    const int nchunk = (L + KC4 - 1) / KC4;
    // the two on-demand global streams of a consumer wave: the raw Q rows of a query tile, the bias of a key tile.  (Requesting them
    // one slot / one tile ahead was measured: no gain with 8 waves of 256 registers, spills with 12 waves - tools/probes/kb_tri.py)
    f32x4 qraw[4], bz[4];
    auto q_load = [&](int qt_) {
        const int qrow_ = qt_ * 16 + lq;
        const bool ok_ = qrow_ < L;
        const float* qp = a.q + base + (long long)(ok_ ? qrow_ : 0) * a.sl;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const bool live = ok_ && (hh == 0 || g < 2);            // d 32..47 only: lane groups 2, 3 of the second step are 0
            qraw[2 * hh] = live ? *reinterpret_cast<const f32x4*>(qp + hh * 32 + g * 8) : (f32x4){0.f, 0.f, 0.f, 0.f};
            qraw[2 * hh + 1] = live ? *reinterpret_cast<const f32x4*>(qp + hh * 32 + g * 8 + 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    // bias of the tile (query tile qt_, chunk at key c0_, keys k0_ + sub*16 + 4g + r of nkeys_ in the chunk)
    auto bias_load = [&](int qt_, int c0_, int nkeys_, int k0_) {
        const int qrow_ = qt_ * 16 + lq;
        const float* brow = biasb ? biasb + (long long)(qrow_ < L ? qrow_ : 0) * a.bias_sq + (long long)c0_ * a.bias_sk : nullptr;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int kq = k0_ + sub * 16 + g * 4;                  // first of this lane's 4 keys (chunk-relative)
            if (bias_vec && c0_ + kq + 4 <= bias_row) {
                bz[sub] = *reinterpret_cast<const f32x4*>(brow + kq);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = min(kq + r, nkeys_ - 1);
                    bz[sub][r] = brow ? brow[(long long)key * a.bias_sk] : 0.f;
                }
            }
        }
    };
    for (int ch = 0; ch < nchunk; ++ch) {
        const int c0 = ch * KC4, buf = DB ? (ch & 1) : 0;
        const int nkeys = min(KC4, L - c0);
        const int nkt = (nkeys + 63) / 64;
        const bool more = DB && ch + 1 < nchunk;
        if (!DB) {
            __syncthreads();                                    // the previous chunk has been consumed
#pragma unroll
            for (int it = 0; it < NIT; ++it) { stage_load(c0, tid + it * NTH); stage_write(c0, 0, tid + it * NTH); }
            if (tid < KC4) stage_mask(c0, 0, tid);
            __syncthreads();
        }
        const char* Kp = lds + buf * BUF4;
        const char* Vp = Kp + 2 * PLN;
        const float* Ms = Msb + buf * KC4;
        const bool masked_chunk = any_masked;                   // (per sample: a masked key anywhere -> clamp every tile)

        if (PROD && wave == NCW) {
            // ---- producer wave: the whole next chunk, 4 (key, 4-channel) items per lane in flight
            if (more) {
                constexpr int NPI = KC4 * (TD / 4) / 64;            // items per lane
                f32x4 kr[4], vr[4];
                for (int j0 = 0; j0 < NPI; j0 += 4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { stage_load(c0 + KC4, lane + (j0 + j) * 64); kr[j] = kreg; vr[j] = vreg; }
#pragma unroll
                    for (int j = 0; j < 4; ++j) { kreg = kr[j]; vreg = vr[j]; stage_write(c0 + KC4, buf ^ 1, lane + (j0 + j) * 64); }
                }
                for (int t = lane; t < KC4; t += 64) stage_mask(c0 + KC4, buf ^ 1, t);
            }
        } else
#pragma unroll
        for (int sl = 0; sl < MAXQ; ++sl) {
            const int qt = qt0 + wave + sl * NCW;
            // (no producer wave) staging item sl of the next chunk rides along with slot sl (slots >= NIT carry none; a wave without a
            // query tile in this slot still does its share)
            if (!PROD && sl < NIT && more) stage_load(c0 + KC4, tid + sl * NTH);
            if (qt < nqt) {
            // ---- Q fragments (B operand of the swapped product), pre-scaled, split: lane holds Q[q][dbase + 8g .. +7]
            f16x8 qf[2][2];
            q_load(qt);
            {
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    float x[8];
                    const f32x4 lo = qraw[2 * hh], hi = qraw[2 * hh + 1];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { x[e] = lo[e] * qscale; x[4 + e] = hi[e] * qscale; }
                    unsigned q0[4], q1[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) split2h_raw(x[2 * e], x[2 * e + 1], q0[e], q1[e]);
                    qf[hh][0] = __builtin_bit_cast(f16x8, u32x4{q0[0], q0[1], q0[2], q0[3]});
                    qf[hh][1] = __builtin_bit_cast(f16x8, u32x4{q1[0], q1[1], q1[2], q1[3]});
                }
            }
            float mr = m_run[sl], lr = l_run[sl];
            f32x4 oo[3] = {o[sl][0], o[sl][1], o[sl][2]};
            using T = SplitTerms;                         // A: the two-piece operand (Q, P), B: the plane operand (K, V)

            for (int kt = 0; kt < nkt; ++kt) {
                const int k0 = kt * 64;
                // ---- bias of this tile (keys k0 + sub*16 + 4g + r): issued first, consumed after the QK^T MFMAs
                bias_load(qt, c0, nkeys, k0);
                f32x4 sc[4];
                // ---- S^T tiles: 4 sub-blocks of 16 keys x 2 d-steps x 6 products
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    const char* kr = Kp + (k0 + sub * 16 + lq) * RST + g * 16;
                    f16x8 ka[2][3];
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        ka[0][p] = *reinterpret_cast<const f16x8*>(kr + p * PLN);
                        // d 32..47: lane groups 0, 1 read d 32 + 8g; groups 2, 3 re-read a valid address and are multiplied by Q = 0
                        ka[1][p] = *reinterpret_cast<const f16x8*>(kr + p * PLN + 64 - (g >> 1) * 32);
                    }
                    ka[0][2] = __builtin_bit_cast(f16x8, f16x8_lo(__builtin_bit_cast(u32x4, ka[0][0])));
                    ka[1][2] = __builtin_bit_cast(f16x8, f16x8_lo(__builtin_bit_cast(u32x4, ka[1][0])));
                    f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int term = 0; term < T::N; ++term)
#pragma unroll
                        for (int hh = 0; hh < 2; ++hh)
                            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka[hh][T::B[term]], qf[hh][T::A[term]], c, 0, 0, 0);
                    sc[sub] = c;
                }
                // ---- bias, mask, online softmax (base 2) of this lane's query column
                float mx;
                // logits (base 2) = S^T + bias * log2(e); the key clamps only where the tile has masked / padded keys
                const bool clamp = masked_chunk || k0 + 64 > nkeys;
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[sub][r] = fmaf(bz[sub][r], bias_l2, sc[sub][r]);
                }
                if (clamp) {
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub) {
                        const f32x4 mk = *reinterpret_cast<const f32x4*>(Ms + k0 + sub * 16 + g * 4);
#pragma unroll
                        for (int r = 0; r < 4; ++r) sc[sub][r] = vmin(sc[sub][r], mk[r]);
                    }
                }
                {   // tree maximum of the lane's 16 logits, then over the 4 lanes of the query column
                    const float m0 = vmax3(sc[0][0], sc[0][1], sc[0][2]), m1 = vmax3(sc[0][3], sc[1][0], sc[1][1]);
                    const float m2 = vmax3(sc[1][2], sc[1][3], sc[2][0]), m3 = vmax3(sc[2][1], sc[2][2], sc[2][3]);
                    const float m4 = vmax3(sc[3][0], sc[3][1], sc[3][2]);
                    mx = vmax(vmax3(m0, m1, m2), vmax3(m3, m4, sc[3][3]));
                }
                mx = quad_max(mx);
                const float m_new = vmax(mr, mx);
                const float alpha = __builtin_amdgcn_exp2f(mr - m_new);
                const float m_sh = m_new + 4.0f;
                float rs4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(sc[sub][r] - m_sh);     // P / 16
                        sc[sub][r] = p;
                        rs4[r] += p;
                    }
                const float rs = quad_sum((rs4[0] + rs4[1]) + (rs4[2] + rs4[3]));
                lr = lr * alpha + rs;
                mr = m_new;
                if (!__all(alpha == 1.0f)) {                        // O^T columns are the queries: lane-local rescale
#pragma unroll
                    for (int d = 0; d < 3; ++d)
#pragma unroll
                        for (int r = 0; r < 4; ++r) oo[d][r] *= alpha;
                }
                // ---- O^T += V^T P: one MFMA step contracts the 32 keys of two sub-blocks; A = V^T (transposing reads of the row-major
                // V planes: lane d receives 8 keys of its column), B = P (registers)
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    f16x8 pa[2];
                    unsigned p0[4], p1[4];
                    split2h_raw(sc[2 * m][0], sc[2 * m][1], p0[0], p1[0]);
                    split2h_raw(sc[2 * m][2], sc[2 * m][3], p0[1], p1[1]);
                    split2h_raw(sc[2 * m + 1][0], sc[2 * m + 1][1], p0[2], p1[2]);
                    split2h_raw(sc[2 * m + 1][2], sc[2 * m + 1][3], p0[3], p1[3]);
                    pa[0] = __builtin_bit_cast(f16x8, u32x4{p0[0], p0[1], p0[2], p0[3]});
                    pa[1] = __builtin_bit_cast(f16x8, u32x4{p1[0], p1[1], p1[2], p1[3]});
                    // lane i of a 16-lane group supplies row (4g + i/4) of the sub-block, 4 channels (i%4)*4.. of the 16-channel block
                    const char* vr = Vp + (k0 + m * 32 + 4 * g + (lq >> 2)) * RST + (lq & 3) * 8;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        f16x8 vb[3];
#pragma unroll
                        for (int p = 0; p < 2; ++p) {
                            const s16x4 lo = lds_tr16(vr + p * PLN + d * 32);
                            const s16x4 hi = lds_tr16(vr + p * PLN + d * 32 + 16 * RST);
                            vb[p] = __builtin_bit_cast(f16x8, s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
                        }
                        vb[2] = __builtin_bit_cast(f16x8, f16x8_lo(__builtin_bit_cast(u32x4, vb[0])));
#pragma unroll
                        for (int term = 0; term < T::N; ++term)
                            oo[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vb[T::B[term]], pa[T::A[term]], oo[d], 0, 0, 0);
                    }
                }
            }
            m_run[sl] = mr;
            l_run[sl] = lr;
            o[sl][0] = oo[0]; o[sl][1] = oo[1]; o[sl][2] = oo[2];
            }
            if (!PROD && sl < NIT && more) {
                stage_write(c0 + KC4, buf ^ 1, tid + sl * NTH);
                if (sl == 0 && tid < KC4) stage_mask(c0 + KC4, buf ^ 1, tid);
            }
        }
        if (DB) __syncthreads();
    }
    if (a.range_flag) {                                         // range safety, see tri_attn8_kernel
        float z = 0.f;
#pragma unroll
        for (int sl = 0; sl < MAXQ; ++sl) {
            const int qt = qt0 + wave + sl * NCW;
            const bool live = wave < NCW && qt < nqt && qt * 16 + lq < L;
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int r = 0; r < 4; ++r) z = fmaf(live ? o[sl][d][r] : 0.f, 0.f, z);
            z = fmaf(live ? l_run[sl] : 0.f, 0.f, z);
        }
        if (__any(z != z) && lane == 0) atomicOr(a.range_flag, a.range_tag);
    }
    // ---- normalise, gate, store.  O^T layout: column = query lq, rows d = dblk*16 + g*4 + r
#pragma unroll
    for (int sl = 0; sl < MAXQ; ++sl) {
        const int qt = qt0 + wave + sl * NCW;
        const int qrow = qt * 16 + lq;
        if (wave >= NCW || qt >= nqt || qrow >= L) continue;
        const float inv = 0.0625f / l_run[sl];                  // l_run accumulated P / 16
        const long long go = base + (long long)qrow * a.sl;
        float* op = a.out + (long long)b * a.ob + (long long)s * a.os + (long long)qrow * a.ol + h * TD;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int dd = d * 16 + g * 4;
            f32x4 v = o[sl][d];
            if (a.gate) {
                const f32x4 gv = *reinterpret_cast<const f32x4*>(a.gate + go + dd);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] * inv * sigmoidf_(gv[r]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] *= inv;
            }
            *reinterpret_cast<f32x4*>(op + dd) = v;
        }
    }
    probe.finish();
}

// One row of tri_attn8: the computing-wave body from the running softmax state to the stored output rows, shared by tri_attn8_kernel (key chunks
// double-buffered by its producer wave, one block barrier per chunk) and tri_attn8_rowfused_kernel (the whole row is one resident chunk: no
// barrier inside), so that the two cannot drift apart.  qf / boff: the query fragments and bias offsets of the wave's two query tiles
// (tri_attn8_kernel loads and splits q, the row-fused kernel takes them from its projection accumulators); cc: chunks consumed so far
// (chunk cc sits in buffer cc & 1).
struct Tri8Row { long long base; const float* km; const float* biasb; int b, h, s, part; };
template <int KC4, bool BVEC, bool CHUNK_BARRIER, class Stamp>
__device__ __forceinline__ void tri8_row_compute(const AbxTriAttn& a, const Tri8Row& cur, const char* lds, const float* Msb, int& cc, const int nchunk,
                                                 const f16x8 (&qf)[2][4], const unsigned (&boff)[2], const bool any_masked, const bool has_tile,
                                                 const int qtA, const int nqt, const int lane, const int koff0, const int koffc, const int voff, Stamp&& stamp) {
    constexpr int PLN = KC4 * RST, BUF4 = 4 * PLN;
    constexpr float SCL = 128.0f, ISCL = 1.0f / 128.0f, PEXP = 8.0f;
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>; using I4 = std::integral_constant<int, 4>;
    const int L = a.L;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 15, g = lane >> 4;
    // running maximum (in accumulator units) and the running sum of the softmax weights: the sums come off the MATRIX pipe as a
    // 49th output channel (A operand = ones: every row of ls is the column sum of the weight pieces the PV product uses) - 8 MFMA
    // issue slots per tile pair instead of the 48 VALU ones of the add tree + the four-lane reduction; the kernel is issue bound
    float mr[2] = {-INFINITY, -INFINITY};
    f32x4 ls[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
    f32x4 oo[2][3];
#pragma unroll
    for (int X = 0; X < 2; ++X)
#pragma unroll
        for (int d = 0; d < 3; ++d) oo[X][d] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // logits of the key tile in flight: bias -> 2^7 (bias log2 e + S^T) -> softmax weights P 2^8 -> (the next tile's bias)
    f32x4 sc[2][4];
    __amdgpu_buffer_rsrc_t brsrc;
    {
        const unsigned long long bu = reinterpret_cast<unsigned long long>(cur.biasb);
        // (readfirstlane returns int: through unsigned, or a low half with bit 31 set sign-extends into the high half)
        const unsigned long long bu_u = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(bu >> 32)) << 32) |
                                        (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)bu);
        brsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(bu_u), 0,
                                                  __builtin_amdgcn_readfirstlane((int)(L * a.bias_sq * 4)), 0x00020000);
    }
    // bias of sub-blocks [S0, S1) of the key tile that starts at key k_abs of the row, into sc
    auto bias_issue = [&](int k_abs, auto s0_, auto s1_) __attribute__((always_inline)) {
        constexpr int S0 = decltype(s0_)::value, S1 = decltype(s1_)::value;
        if (BVEC) {
            // buffer loads: the pair's (L, Lp) bias as the resource (wave-uniform descriptor), (query row, key) in the per-lane 32-bit
            // offset, the sub-block as immediate: no 64-bit vector address arithmetic.  Keys beyond the padded row read the next row's
            // floats (beyond the matrix: the range check returns 0): replaced by the -inf clamp
            // (the tile's first key goes into the per-lane offset, not the scalar one: only the former is range-checked)
#pragma unroll
            for (int X = 0; X < 2; ++X) {
                const unsigned vo = boff[X] + (unsigned)k_abs * 4u;
#pragma unroll
                for (int sub = S0; sub < S1; ++sub)
                    sc[X][sub] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brsrc, vo + sub * 64, 0, 0));
            }
        } else {
#pragma unroll
            for (int X = 0; X < 2; ++X)
#pragma unroll
                for (int sub = S0; sub < S1; ++sub) {
                    const int kq = k_abs + sub * 16 + g * 4;
                    const float* brow = cur.biasb ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(cur.biasb) + boff[X]) - g * 4 : nullptr;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        sc[X][sub][r] = brow ? brow[(long long)min(kq + r, L - 1) * a.bias_sk] : 0.f;
                }
        }
    };
    if (has_tile) bias_issue(0, I0{}, I4{});
    if (wave == 0) stamp();

    for (int ch = 0; ch < nchunk; ++ch, ++cc) {
        const int c0 = ch * KC4, buf = cc & 1;
        const int nkeys = min(KC4, L - c0);
        const int nkt = (nkeys + 63) / 64;
        const bool more = ch + 1 < nchunk;
        const char* Kp = lds + buf * BUF4;
        const char* Vp = Kp + 2 * PLN;
        const float* Ms = Msb + buf * KC4;
        if (has_tile)
        for (int kt = 0; kt < nkt; ++kt) {
            const int k0 = kt * 64;
            const bool full = nkeys - k0 > 32;              // otherwise: sub-blocks 0, 1 and the first PV step only
            // next key tile of this row (its bias is requested under the PV work below): first key, or -1
            const int k_next = kt + 1 < nkt ? c0 + k0 + 64 : (more ? c0 + KC4 : -1);
            if ((BVEC || cur.biasb) && !a.bias_log2) {      // (bias_log2: the projection applied the factor, AbxGemm.alpha)
#pragma unroll
                for (int X = 0; X < 2; ++X)
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sc[X][sub][r] *= LOG2E * SCL;
            }
            // ---- S^T tiles (accumulators start from the bias): terms a1 p0, a0 p1, a0 p0, smallest first
            auto qk = [&](auto sub_) __attribute__((always_inline)) {
                constexpr int sub = decltype(sub_)::value;
                const char* kr = Kp + (k0 + sub * 16) * RST;
                const f16x8 r0 = *reinterpret_cast<const f16x8*>(kr + koff0);
                const f16x8 r1 = *reinterpret_cast<const f16x8*>(kr + koff0 + PLN);
                const f16x8 rc = *reinterpret_cast<const f16x8*>(kr + koffc);
#pragma unroll
                for (int X = 0; X < 2; ++X) sc[X][sub] = __builtin_amdgcn_mfma_f32_16x16x32_f16(r0, qf[X][1], sc[X][sub], 0, 0, 0);
#pragma unroll
                for (int X = 0; X < 2; ++X) sc[X][sub] = __builtin_amdgcn_mfma_f32_16x16x32_f16(rc, qf[X][3], sc[X][sub], 0, 0, 0);
#pragma unroll
                for (int X = 0; X < 2; ++X) sc[X][sub] = __builtin_amdgcn_mfma_f32_16x16x32_f16(r1, qf[X][0], sc[X][sub], 0, 0, 0);
#pragma unroll
                for (int X = 0; X < 2; ++X) sc[X][sub] = __builtin_amdgcn_mfma_f32_16x16x32_f16(rc, qf[X][2], sc[X][sub], 0, 0, 0);
#pragma unroll
                for (int X = 0; X < 2; ++X) sc[X][sub] = __builtin_amdgcn_mfma_f32_16x16x32_f16(r0, qf[X][0], sc[X][sub], 0, 0, 0);
            };
            qk(I0{});
            qk(I1{});
            if (full) {
                qk(I2{});
                qk(I3{});
            } else {
#pragma unroll
                for (int X = 0; X < 2; ++X) {
                    sc[X][2] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    sc[X][3] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                }
            }
            // ---- key clamps (masked / padded keys), online softmax (base 2) of this lane's query columns
            if (any_masked || k0 + 64 > nkeys) {
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    const f32x4 mk = *reinterpret_cast<const f32x4*>(Ms + k0 + sub * 16 + g * 4);
#pragma unroll
                    for (int X = 0; X < 2; ++X)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sc[X][sub][r] = vmin(sc[X][sub][r], mk[r]);
                }
            }
#pragma unroll
            for (int X = 0; X < 2; ++X) {
                const float m0 = vmax3(sc[X][0][0], sc[X][0][1], sc[X][0][2]), m1 = vmax3(sc[X][0][3], sc[X][1][0], sc[X][1][1]);
                const float m2 = vmax3(sc[X][1][2], sc[X][1][3], sc[X][2][0]), m3 = vmax3(sc[X][2][1], sc[X][2][2], sc[X][2][3]);
                const float m4 = vmax3(sc[X][3][0], sc[X][3][1], sc[X][3][2]);
                const float mx = quad_max(vmax(vmax3(m0, m1, m2), vmax3(m3, m4, sc[X][3][3])));
                const float m_new = vmax(mr[X], mx);
                const float alpha = __builtin_amdgcn_exp2f((mr[X] - m_new) * ISCL);
                const float m_sh = PEXP - m_new * ISCL;
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[X][sub][r] = __builtin_amdgcn_exp2f(fmaf(sc[X][sub][r], ISCL, m_sh));     // P 2^8
                mr[X] = m_new;
                if (!__all(alpha == 1.0f)) {                    // O^T columns are the queries: lane-local rescale
#pragma unroll
                    for (int d = 0; d < 3; ++d)
#pragma unroll
                        for (int r = 0; r < 4; ++r) oo[X][d][r] *= alpha;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ls[X][r] *= alpha;
                }
            }
            // ---- O^T += V^T P: one step contracts the 32 keys of two sub-blocks; the bias of the next tile goes into the
            // registers the weights leave
            auto pv = [&](auto m_) __attribute__((always_inline)) {
                constexpr int m = decltype(m_)::value;
                f16x8 pa[2][2];
#pragma unroll
                for (int X = 0; X < 2; ++X) {
                    unsigned p0[4], p1[4];
                    split2h_ns(sc[X][2 * m][0], sc[X][2 * m][1], p0[0], p1[0]);
                    split2h_ns(sc[X][2 * m][2], sc[X][2 * m][3], p0[1], p1[1]);
                    split2h_ns(sc[X][2 * m + 1][0], sc[X][2 * m + 1][1], p0[2], p1[2]);
                    split2h_ns(sc[X][2 * m + 1][2], sc[X][2 * m + 1][3], p0[3], p1[3]);
                    pa[X][0] = __builtin_bit_cast(f16x8, u32x4{p0[0], p0[1], p0[2], p0[3]});
                    pa[X][1] = __builtin_bit_cast(f16x8, u32x4{p1[0], p1[1], p1[2], p1[3]});
                }
                if (k_next >= 0) bias_issue(k_next, std::integral_constant<int, 2 * m>{}, std::integral_constant<int, 2 * m + 2>{});
                {
                    const _Float16 one = (_Float16)1.0f;
                    const f16x8 ones = {one, one, one, one, one, one, one, one};
#pragma unroll
                    for (int X = 0; X < 2; ++X) ls[X] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pa[X][1], ls[X], 0, 0, 0);
#pragma unroll
                    for (int X = 0; X < 2; ++X) ls[X] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pa[X][0], ls[X], 0, 0, 0);
                }
                const char* vr = Vp + (k0 + m * 32) * RST + voff;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    f16x8 vb[2];
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        const s16x4 lo = lds_tr16(vr + p * PLN + d * 32);
                        const s16x4 hi = lds_tr16(vr + p * PLN + d * 32 + 16 * RST);
                        vb[p] = __builtin_bit_cast(f16x8, s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
                    }
#pragma unroll
                    for (int X = 0; X < 2; ++X) oo[X][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vb[0], pa[X][1], oo[X][d], 0, 0, 0);
#pragma unroll
                    for (int X = 0; X < 2; ++X) oo[X][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vb[1], pa[X][0], oo[X][d], 0, 0, 0);
#pragma unroll
                    for (int X = 0; X < 2; ++X) oo[X][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vb[0], pa[X][0], oo[X][d], 0, 0, 0);
                }
            };
            pv(I0{});
            if (full) {
                pv(I1{});
            } else if (k_next >= 0) {
                bias_issue(k_next, I2{}, I4{});             // (a half tile is the last of its row: not reached)
            }
        }
        if (wave == 0) stamp();
        if (CHUNK_BARRIER) __syncthreads();
        if (wave == 0) stamp();
    }
    bool bad = false;           // range safety (AbxTriAttn.range_flag): a key / value / query / gate beyond the split ranges, or not finite
    // ---- normalise, gate, store.  O^T layout: column = query lq, rows d = dblk*16 + g*4 + r
#pragma unroll
    for (int X = 0; X < 2; ++X) {
        const int qrow = (qtA + X) * 16 + lq;
        if (qtA + X >= nqt || qrow >= L) continue;
        const float inv = 0.0625f / ls[X][0];               // O^T accumulated (16 v) (P 2^8), ls = sum P 2^8 (every row)
        const long long go = cur.base + (long long)qrow * a.sl;
        float* op = a.out + (long long)cur.b * a.ob + (long long)cur.s * a.os + (long long)qrow * a.ol + cur.h * TD;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int dd = d * 16 + g * 4;
            f32x4 v = oo[X][d];
            if (a.gate) {
                const f32x4 gv = *reinterpret_cast<const f32x4*>(a.gate + go + dd);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] * inv * sigmoidf_(gv[r]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] *= inv;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) bad |= __builtin_amdgcn_classf(v[r], 0x207);
            *reinterpret_cast<f32x4*>(op + dd) = v;
        }
    }
    if (a.range_flag && __any(bad) && lane == 0) atomicOr(a.range_flag, a.range_tag);
}


// ---- triangle attention, paired query tiles (split-f16) ----------------------------------------------------------------------
// Same (b, row, head) decomposition and LDS image as tri_attn4_kernel (K / V of a row staged in key chunks as two f16 planes each,
// swapped S^T = K Q^T, transposing V reads, online base-2 softmax per query column).  What is different:
//   * PERSISTENT workgroups: the grid is one workgroup per CU, workgroup j of XCD x walks the slots j, j + 32, ... of that XCD's
//     (b, h, row) list (so the 32 CUs of an XCD still work on neighbouring rows of ONE (b, h) pair: its bias stays in that L2), and
//     the PRODUCER wave streams key chunks across row boundaries: while the 11 computing waves work on the last chunk of a row it
//     stages the first chunk of the next one.  One workgroup owns a CU (99 / 147 KB of LDS), so in the one-row-per-workgroup form
//     nothing ran under a row's prologue (K / V of chunk 0 from HBM, first barrier) and under the dispatch of the next workgroup:
//     a third of the kernel.
//   * a computing wave walks its TWO query tiles (2w, 2w + 1 of the row's <= 22) together over the key tiles: every K / V fragment
//     read serves two S^T / O^T tiles (half the LDS fragment traffic per product) and the matrix pipe sees two independent
//     accumulator chains (a wave whose second tile lies beyond the row computes it on the clamped last query row and drops it);
//   * the Q fragments of both tiles are loaded and split ONCE per row;
//   * the pair bias is the INITIAL VALUE of the S^T accumulators: the loads of the next key tile's bias go into the registers the
//     softmax weights of this tile have just left, under the PV matrix work;
//   * operand scales chosen so that the second piece of a query / softmax weight needs no 2^11 lift: the three product terms use the
//     stored planes p0, p1 as they are (no p2 = p0 2^-11 derivation);
//   * the 48-wide head is 32 + 16 channels: the second k-step carries BOTH plane terms of channels 32..47 (lane groups 0, 1 read
//     p0, groups 2, 3 read p1 of the same 16 channels, the query piece a0 is held twice): 5 matrix instructions per 16-key
//     sub-block instead of 6, 3 fragment reads instead of 4;
//   * a last key tile with <= 32 keys runs half a tile.
// The kernel is instruction-issue bound (one paired tile step: 76 MFMA + ~300 VALU + 36 LDS per wave, three waves per SIMD).
// Rows with more than 22 query tiles are dealt to q_parts slots.
// BVEC: the bias rows are key-contiguous, 16-byte aligned and padded to a multiple of 4 floats (what model/forward.py passes): one
// 16-byte load per sub-block; otherwise (any strides, or no bias) the generic element loads
template <int KC4, int NTH, bool BVEC>
__global__ __launch_bounds__(NTH) void tri_attn8_kernel(const AbxTriAttn a) {
    constexpr int PLN = KC4 * RST;           // bytes per plane
    constexpr int BUF4 = 4 * PLN;            // K planes + V planes (p0, p1) of one chunk
    constexpr int NCW = NTH / 64 - 1;        // computing waves; the last wave is the producer
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* lds = reinterpret_cast<char*>(smem);
    float* Msb = reinterpret_cast<float*>(lds + 2 * BUF4);       // [2][KC4] key-mask clamps of the chunks in flight
    const int L = a.L;
    const ClockProbe probe(a.clock_probe);
#ifdef TRI8_STAMP
    // diagnostic build: shader-clock stamps of wave 0 (slots 0..15) and of the producer wave (16..31) while the workgroup is on its
    // FOURTH row (steady state), one record per workgroup
    unsigned long long* st_buf = a.clock_probe ? a.clock_probe + 16 + (size_t)blockIdx.x * 32 : nullptr;
    int st_n = 0, st_row = 0;
#define STAMP() { if (st_buf && st_row == 3 && (threadIdx.x & 63) == 0 && st_n < 16) st_buf[(threadIdx.x >= NCW * 64 ? 16 : 0) + st_n] = __builtin_amdgcn_s_memtime(); if (st_row == 3) ++st_n; }
#else
#define STAMP() {}
#endif
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 15, g = lane >> 4;
    // ---- the slots of this workgroup: XCD x = blockIdx & 7 owns the virtual pairs x, x + 8, ...; a slot is (pair, row, part)
    const int xcd = blockIdx.x & 7, wg = blockIdx.x >> 3, NW = gridDim.x >> 3;
    const int G = a.row_groups, rows_g = (a.S + G - 1) / G;
    const int per_vp = rows_g * a.q_parts;
    const int nvp = a.B * a.H * G;
    const long long nslots = (long long)((nvp - xcd + 7) / 8) * per_vp;          // slots of this XCD
    using Row = Tri8Row;
    auto decode = [&](long long slot, Row& r) __attribute__((always_inline)) -> bool {
        const int sp = (int)(slot % per_vp), vp = (int)(slot / per_vp) * 8 + xcd;
        const int bh = vp / G;
        r.s = (sp / a.q_parts) * G + vp % G;
        r.part = sp % a.q_parts;
        if (r.s >= a.S) return false;                                              // (ragged last row group)
        r.b = bh / a.H;
        r.h = bh % a.H;
        // (wave-uniform, but the divisions above run on the vector unit: back to scalar registers - the producer wave holds two rows)
        r.b = __builtin_amdgcn_readfirstlane(r.b);
        r.h = __builtin_amdgcn_readfirstlane(r.h);
        r.s = __builtin_amdgcn_readfirstlane(r.s);
        r.part = __builtin_amdgcn_readfirstlane(r.part);
        r.base = (long long)r.b * a.sb + (long long)r.s * a.ss + (long long)r.h * TD;
        r.km = a.keymask ? a.keymask + (long long)r.b * a.km_sb : nullptr;
        r.biasb = a.bias ? a.bias + (long long)r.b * a.bias_sb + (long long)r.h * a.bias_sh : nullptr;
        return true;
    };
    auto next_slot = [&](long long slot, Row& r) __attribute__((always_inline)) -> long long {       // first valid slot >= slot, or -1
        for (; slot < nslots; slot += NW)
            if (decode(slot, r)) return slot;
        return -1;
    };
    const int nchunk = (L + KC4 - 1) / KC4;
    const int nqt_row = (L + 15) / 16, tpp = (nqt_row + a.q_parts - 1) / a.q_parts;

    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;

    if (wave == NCW) {
        // ================= producer wave: K / V of the chunk after the one being computed, across row boundaries ==============
        // (the last-dispatched wave of the workgroup loses every VALU / LDS issue arbitration against the older computing waves of
        // its SIMD, and it is the one the chunk barrier waits for: static priority)
        __builtin_amdgcn_s_setprio(3);
        // per-lane constants of the staging: item j of a round is (key kk0[j] + 32 rd, 4-channel group c4) with idx = lane + 64 j =
        // 12 kk0 + c4 (a round of 6 items advances every key by 384 / 12 = 32): LDS byte offset inside a plane, byte offset inside a row
        constexpr int NPI = KC4 * (TD / 4) / 64;                // (key, 4-channel) items per lane: 36 (192-key chunks) / 24
        constexpr int NPF = 6, NRD = NPI / NPF;                 // rounds of 6 items (12 loads of 16 bytes per lane)
        static_assert(NPI % NPF == 0 && NRD % 2 == 0 && (NPF * 64) % (TD / 4) == 0, "rounds");
        constexpr int KRD = NPF * 64 / (TD / 4);                // keys a round advances: 32
        const unsigned sl4 = (unsigned)(a.sl * 4);             // row stride in bytes (< 2^24, rows of one (b, s) slab < 4 GB: the dispatch)
        float c16 = 16.0f;                                      // (VOP3P takes no literal; a VGPR: see split2b_mix)
        asm volatile("" : "+v"(c16));
        auto stage = [&](const Row& r, int c0, int buf) __attribute__((always_inline)) {
            char* Kp = lds + buf * BUF4;
            char* Vp = Kp + 2 * PLN;
            if (a.kv_planes) {
                // Round 6: k | v arrive as the operand images the projection wrote (AbxGemm.c_planes_from: per key and head [p0: 48 f16 | p1: 48
                // f16] of 16 x value, at the byte address of the fp32 head slice).  A plane of the chunk is a dense [KC4][96 bytes] array in
                // LDS, so staging is a straight DMA: instruction i of a plane fills bytes [1024 i, 1024 i + 1024) - lane l the 16 bytes at
                // o = 1024 i + 16 l = (key o / 96, byte o % 96); three instructions cover 32 keys exactly, so a lane has three (key, byte)
                // constants.  No registers, no split, no LDS writes by this wave: 4 planes x PLN / 1024 instructions per chunk, one wait.
                constexpr int NI = PLN / 1024;
                static_assert(PLN % 3072 == 0, "a plane of the chunk is a whole number of 32-key DMA rounds");
                int ln = lane;
                asm volatile("" : "+v"(ln));                     // (per chunk, behind an opaque lane id: see the staging constants below)
                const char* kb = reinterpret_cast<const char*>(a.k + r.base);
                const char* vb = reinterpret_cast<const char*>(a.v + r.base);
                int kt[3];
                unsigned cb[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int o = t * 1024 + ln * 16;
                    kt[t] = o / RST;
                    cb[t] = (unsigned)(o - kt[t] * RST);
                }
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const unsigned off = __umul24((unsigned)min(c0 + 32 * (i / 3) + kt[i % 3], L - 1), sl4) + cb[i % 3];
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        glds16(kb + off + p * RST, Kp + p * PLN + i * 1024);
                        glds16(vb + off + p * RST, Vp + p * PLN + i * 1024);
                    }
                }
                for (int t = lane; t < KC4; t += 64)
                    Msb[buf * KC4 + t] = (c0 + t < L) ? ((!r.km || r.km[c0 + t] != 0.f) ? INFINITY : ABX_NEG_MAX) : -INFINITY;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the images have landed before this wave joins the chunk barrier)
                return;
            }
            // (recomputed per chunk behind an opaque lane id: as invariants of the whole kernel they are hoisted above the wave-role
            // branch and cost the computing waves 18 registers - spills)
            int ln = lane;
            asm volatile("" : "+v"(ln));
        int kk0[NPF];
        unsigned ldo[NPF], gco[NPF];
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            const int idx = ln + j * 64;
            kk0[j] = idx / (TD / 4);
            ldo[j] = (unsigned)(kk0[j] * RST + (idx % (TD / 4)) * 8);
            gco[j] = (unsigned)((idx % (TD / 4)) * 16);
        }
            // wave-uniform slab bases + 32-bit per-lane offsets (scalar-base loads: no 64-bit vector address arithmetic per item)
            const char* kb = reinterpret_cast<const char*>(a.k + r.base);
            const char* vb = reinterpret_cast<const char*>(a.v + r.base);
            // software pipeline over the rounds: the loads of round rd + 1 are in flight while round rd is split and written
            f32x4 kr[2][NPF], vr[2][NPF];
            auto issue = [&](int rd, auto set_) __attribute__((always_inline)) {
                constexpr int set = decltype(set_)::value;
#pragma unroll
                for (int j = 0; j < NPF; ++j) {
                    // UNCONDITIONAL loads (a conditional one makes the number of loads in flight unknown to the compiler: it then waits
                    // for vmcnt(0) before the previous round's values, and the pipeline is gone).  Keys beyond L re-read the last key:
                    // their logits are clamped to -inf (Msb), their softmax weights are exactly 0 against a finite V row
                    const unsigned off = __umul24((unsigned)min(c0 + rd * KRD + kk0[j], L - 1), sl4) + gco[j];
                    // read once per launch: non-temporal, so that the K / V stream does not push the pair's bias out of the L2
#ifdef TRI8_TEMPORAL                                                    // (probe: plain loads)
                    kr[set][j] = *reinterpret_cast<const f32x4*>(kb + off);
                    vr[set][j] = *reinterpret_cast<const f32x4*>(vb + off);
#else
                    kr[set][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(kb + off));
                    vr[set][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vb + off));
#endif
                }
            };
            auto convert = [&](int rd, auto set_) __attribute__((always_inline)) {
                constexpr int set = decltype(set_)::value;
                const unsigned rdo = (unsigned)(rd * KRD * RST);
#ifdef TRI8_LOADS_ONLY     // (probe build: every K / V load still issues and is waited for, but nothing is split or written except one word per
                           //  round - the kernel's time with the HBM stream and without the producer's VALU / LDS work: what DMA staging could return)
                unsigned x = 0;
#pragma unroll
                for (int j = 0; j < NPF; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) x ^= __builtin_bit_cast(unsigned, kr[set][j][e]) ^ __builtin_bit_cast(unsigned, vr[set][j][e]);
                *reinterpret_cast<unsigned*>(Kp + rdo + ldo[0]) = x;
                return;
#endif
#pragma unroll
                for (int j = 0; j < NPF; ++j) {
                    unsigned a0, a1, b0, b1;
                    split2b_mix(kr[set][j][0], kr[set][j][1], c16, a0, a1);
                    split2b_mix(kr[set][j][2], kr[set][j][3], c16, b0, b1);
                    char* kd = Kp + rdo + ldo[j];
                    *reinterpret_cast<u32x2*>(kd) = u32x2{a0, b0};
                    *reinterpret_cast<u32x2*>(kd + PLN) = u32x2{a1, b1};
                    split2b_mix(vr[set][j][0], vr[set][j][1], c16, a0, a1);
                    split2b_mix(vr[set][j][2], vr[set][j][3], c16, b0, b1);
                    char* vd = Vp + rdo + ldo[j];
                    *reinterpret_cast<u32x2*>(vd) = u32x2{a0, b0};
                    *reinterpret_cast<u32x2*>(vd + PLN) = u32x2{a1, b1};
                }
            };
#ifndef TRI8_NO_PRODUCER   // (probe build, tools/probes/build_noprod.sh: no K / V staging at all - wrong results, the kernel's time without
                           //  any producer work: the ceiling of what staging by DMA from pre-split planes could return)
            // (a real loop over round pairs; scheduling barriers: the compiler would hoist every round's loads to the top and spill)
            issue(0, I0{});
#pragma unroll 1
            for (int rd = 0; rd < NRD - 2; rd += 2) {           // (every issue unconditional: see above)
                issue(rd + 1, I1{});
                __builtin_amdgcn_sched_barrier(0);
                convert(rd, I0{});
                __builtin_amdgcn_sched_barrier(0);
                issue(rd + 2, I0{});
                __builtin_amdgcn_sched_barrier(0);
                convert(rd + 1, I1{});
                __builtin_amdgcn_sched_barrier(0);
            }
            issue(NRD - 1, I1{});
            __builtin_amdgcn_sched_barrier(0);
            convert(NRD - 2, I0{});
            __builtin_amdgcn_sched_barrier(0);
            convert(NRD - 1, I1{});
            __builtin_amdgcn_sched_barrier(0);
#endif
            // key clamps, applied as logit = min(logit, clamp): +inf valid, finfo.min masked (the reference REPLACES the logit by
            // finfo.min: every finite logit is >= finfo.min), -inf beyond L
            for (int t = lane; t < KC4; t += 64)
                Msb[buf * KC4 + t] = (c0 + t < L) ? ((!r.km || r.km[c0 + t] != 0.f) ? INFINITY : ABX_NEG_MAX) : -INFINITY;
        };
        Row cur, nxt;
        long long slot = next_slot(wg, cur);
        int cc = 0;                                             // chunks staged so far: chunk cc goes to buffer cc & 1
        if (slot >= 0) stage(cur, 0, 0);
        __syncthreads();
        while (slot >= 0) {
            const long long slot2 = next_slot(slot + NW, nxt);
            for (int ch = 0; ch < nchunk; ++ch) {
                ++cc;
                STAMP()
                if (ch + 1 < nchunk) stage(cur, (ch + 1) * KC4, cc & 1);
                else if (slot2 >= 0) stage(nxt, 0, cc & 1);
                STAMP()
                __syncthreads();
            }
            STAMP()
#ifdef TRI8_STAMP
            ++st_row;
#endif
            slot = slot2;
            cur = nxt;
        }
        probe.finish();
        return;
    }

    // ================= computing waves ======================================================================================
    // scales (powers of two: exact): keys / values are staged as 16 x (planes p0, p1 = f16(x'), f16(x' - p0)); queries enter as
    // q scale log2(e) 2^3, so the S^T accumulators hold 2^7 x the base-2 logits; softmax weights as P 2^8.  With these scales the
    // second piece of a query / weight, f16(x' - f16(x')), needs no 2^11 lift (a float16 subnormal only below |x'| = 2^-2, where its
    // 2^-25 absolute error is far below the rounding of the neighbouring products), so the three product terms a1 p0 + a0 p1 + a0 p0
    // use the stored planes as they are
    const float qscale = a.scale * LOG2E * 8.0f;
    const int koff0 = lq * RST + g * 16;                                  // K fragment, channels 8g .. (plane p: + p PLN)
    const int koffc = lq * RST + (g >> 1) * PLN + 64 + (g & 1) * 16;      // channels 32 + 8(g&1) .. of plane g >> 1
    const int voff = (4 * g + (lq >> 2)) * RST + (lq & 3) * 8;            // transposing V reads (see tri_attn4_kernel)

    Row cur;
    long long slot = next_slot(wg, cur);
    int cc = 0;                                                 // chunks consumed so far
    bool any_masked = false;
    int b_masked = -1;
    __syncthreads();                                            // the first chunk of the first row is staged
    while (slot >= 0) {
        const int qt0 = cur.part * tpp, nqt = min(nqt_row, qt0 + tpp);
        const int qtA = qt0 + 2 * wave;
        const bool has_tile = qtA < nqt;                        // (a wave without tiles still joins the barriers)
        if (wave == 0) STAMP()
        if (cur.b != b_masked) {                                // wave-uniform: does this sample mask any key?  (once per sample: the
            any_masked = false;                                 // rows of a workgroup walk one (b, h) pair before the next)
            if (cur.km) {
                for (int j = lane; j < L; j += 64) any_masked |= cur.km[j] == 0.f;
                any_masked = __any(any_masked);
            }
            b_masked = cur.b;
        }
        // ---- Q fragments (B operand of the swapped product), pre-scaled, split once per row.
        // qf[X][0], [1]: pieces a0, a1 of channels 8g .. 8g+7 (first k-step); qf[X][2]: a0 of channels 32 + 8(g&1) .. (second k-step:
        // held by groups g and g + 2, against p0 | p1); qf[X][3]: a1 of the same channels in groups 0, 1, zero in groups 2, 3
        f16x8 qf[2][4];
        unsigned boff[2];                                        // byte offset of (query row, key 4g) inside the pair's bias (< 4 GB)
#pragma unroll
        for (int X = 0; X < 2; ++X) {
            const int qrow = min((qtA + X) * 16 + lq, L - 1);     // beyond the row: the last query row again (never stored)
            const float* qp = a.q + cur.base + (long long)qrow * a.sl;
            boff[X] = (unsigned)(((long long)qrow * a.bias_sq + g * 4) * 4);
            const f32x4 q0 = *reinterpret_cast<const f32x4*>(qp + g * 8);
            const f32x4 q1 = *reinterpret_cast<const f32x4*>(qp + g * 8 + 4);
            const f32x4 q2 = *reinterpret_cast<const f32x4*>(qp + 32 + (g & 1) * 8);
            const f32x4 q3 = *reinterpret_cast<const f32x4*>(qp + 32 + (g & 1) * 8 + 4);
            unsigned p0[4], p1[4];
            split2h_ns(q0[0] * qscale, q0[1] * qscale, p0[0], p1[0]);
            split2h_ns(q0[2] * qscale, q0[3] * qscale, p0[1], p1[1]);
            split2h_ns(q1[0] * qscale, q1[1] * qscale, p0[2], p1[2]);
            split2h_ns(q1[2] * qscale, q1[3] * qscale, p0[3], p1[3]);
            qf[X][0] = __builtin_bit_cast(f16x8, u32x4{p0[0], p0[1], p0[2], p0[3]});
            qf[X][1] = __builtin_bit_cast(f16x8, u32x4{p1[0], p1[1], p1[2], p1[3]});
            split2h_ns(q2[0] * qscale, q2[1] * qscale, p0[0], p1[0]);
            split2h_ns(q2[2] * qscale, q2[3] * qscale, p0[1], p1[1]);
            split2h_ns(q3[0] * qscale, q3[1] * qscale, p0[2], p1[2]);
            split2h_ns(q3[2] * qscale, q3[3] * qscale, p0[3], p1[3]);
            qf[X][2] = __builtin_bit_cast(f16x8, u32x4{p0[0], p0[1], p0[2], p0[3]});
            qf[X][3] = g < 2 ? __builtin_bit_cast(f16x8, u32x4{p1[0], p1[1], p1[2], p1[3]}) : __builtin_bit_cast(f16x8, u32x4{0u, 0u, 0u, 0u});
        }
        tri8_row_compute<KC4, BVEC, true>(a, cur, lds, Msb, cc, nchunk, qf, boff, any_masked, has_tile, qtA, nqt, lane, koff0, koffc, voff,
                                          [&]() __attribute__((always_inline)) { STAMP() });
        if (wave == 0) STAMP()
#ifdef TRI8_STAMP
        ++st_row;
#endif
        slot = next_slot(slot + NW, cur);
    }
#undef STAMP
    probe.finish();
}

// ---- triangle attention with the q | k | v projection of the row inside (split-f16) ------------------------------------------------
// tri_attn8_kernel reads q | k | v of a pair row (b, s) from memory, where the LayerNorm -> Linear projection (gemm_as.hip) has just put
// them: 576 fp32 per pair position written and read back, 57 GB per launch at 100 samples of L = 352, for values only this row's
// attention consumes (seqformer.py:527-548).  Here a slot (b, row s, head h) has two phases:
//   P  wave w projects the 32 positions 32 w .. 32 w + 31 of the row (its two query tiles of phase A): [k_h | v_h | q_h] =
//      LN(z[b, s, l, :]) W_h with the arithmetic of gemm_as / gemm3_mainloop - the pieces of split2h_mix on the shifted row, the shifted
//      statistics summed in k-tile order, the terms a1 p2, a0 p1, a0 p0 per k-step, v_mfma_f32_32x32x16_f16, the folded-LayerNorm epilogue
//      rs (acc - dmean csum / cs) + bias - with the operands SWAPPED as in gemm3_mlp_block: a lane holds ONE position and 16 channels of
//      a 32-column tile, so the row statistics are lane-local.  The walk is k-group outer: the wave holds the pieces of four k-tiles (32
//      registers; all twelve - 96 - next to one accumulator set spilled) and the accumulators of all five column tiles (80; phase A's are
//      not live yet), and re-reads its rows from the L2 per k-group.  k and v leave through split2b_mix straight into the K / V planes of tri_attn8 in LDS
//      (16-byte stores: the head's columns are packed so that a lane holds 8 consecutive channels); q stays in registers: the pack gives
//      lane half hh the channels 16 hh .. 16 hh + 15 and BOTH halves the channels 32 .. 47, so the fragments (query lq, group g) of the
//      wave's two query tiles are one v_permlane16_swap per value away.
//      The head's weight planes (AbxTriRowPack: per head 15 stages of 8 KB = (4 k-tiles, column tile) in LDS fragment order) arrive by
//      global_load_lds, issued by the twelfth wave (at L <= 352 it has no rows): the first three stages into a 24 KB ring while the
//      computing waves are still in phase A of the previous slot, the other twelve into the plane region, which is empty until the tile
//      epilogues write K / V.  Five block barriers per slot (see the issuing wave); a barrier per stage cost 0.8 ms per launch more.
//      The issuing wave can also touch the z row ahead of the walk (TriRowArgs.touch, tri_row_touch.h), so that the projection starts
//      from the L2; measured, every touch schedule loses to none (RF_DEFAULT_TOUCH).
//   A  tri8_row_compute on the resident row (one "chunk"), no barrier inside.
// Every product, sum and rounding is the one the two launches perform: the output is bit-identical to gemm_as + tri_attn8.
// Slot order (TriRowArgs.order): 0 = (b, row, h) with the four heads of a row on neighbouring workgroups of one XCD (the 270 KB of
// z[b, s] come from HBM once and from that L2 three times; the XCD keeps four bias maps hot), 1 = (b, h, row) as tri_attn8.
constexpr int RF_LK = 352;                                   // keys the planes hold: the largest eligible row
constexpr int RF_PLN = RF_LK * RST;                          // 33 792
constexpr int RF_OFF_MSB = 4 * RF_PLN;                       // key clamps [384]
constexpr int RF_OFF_RING = RF_OFF_MSB + 384 * 4;            // 136 704
constexpr int RF_STAGE = 8192;                               // [4 k-tiles][2 planes][32 columns][16] f16
constexpr int RF_NRING = 3;                                 // stages the ring holds
constexpr int RF_G0 = RF_NRING;                             // stages of a slot requested ahead into the ring; the others go through the plane region
constexpr int RF_OFF_CONST = RF_OFF_RING + RF_NRING * RF_STAGE;      // [csum 160 | bias 160] of the slot's head, packed column order
constexpr int RF_LDS = RF_OFF_CONST + 2 * 160 * 4;           // 162 560 <= 163 840
constexpr int RF_TILES = 5, RF_SPS = 3 * RF_TILES;           // column tiles (160 packed columns), stages per slot
constexpr int RF_HEAD_BYTES = RF_SPS * RF_STAGE;             // 122 880 per head
constexpr int RF_DEFAULT_ORDER = 0;                          // slot order of slot_order = -1 (AbxTriRowPack / abx_tri_attn_rowfused_fwd)
constexpr int RF_NK = 12;                                    // k-tiles: 192 input channels
// The issuing wave's counted waits.  Its vector-memory queue behind barrier (a) holds the DMA instructions of G1 and G2 (RF_VM_GROUP each) and,
// with TriRowArgs.touch == 2, the RFT_N touch loads of k-group 1 between them and those of k-group 2 behind barrier (b); results return
// in issue order, so "G1 landed" = at most G2 and the touches in flight, "G2 landed" = at most the touches of k-group 2.
constexpr int RF_VM_GROUP = (RF_SPS - RF_G0) / 2 * (RF_STAGE / 1024);       // 48 DMA instructions per group
constexpr int RF_VM_B = RF_VM_GROUP, RF_VM_C = 0;                           // barriers (b), (c) without touches inside phase P
constexpr int RF_VM_B_JIT = RF_VM_GROUP + RFT_N, RF_VM_C_JIT = RFT_N;       // touch == 2: 60, 12
static_assert(RF_VM_B_JIT <= 63, "vmcnt is a 6-bit count");
static_assert(RF_LK == RFT_LMAX && RF_NK * 16 == RFT_CH && RF_NK == 4 * RFT_KGROUPS, "tri_row_touch.h describes this walk");
// TriRowArgs.touch without ABX_TRI_ROW_TOUCH / abx_tri_row_touch: no touch.  On the counters the whole-row touch (1) costs 9.2 GB of reads per
// launch at 100 samples of L = 352 (its lines are gone before the walks reach them) and 1 ms; the just-in-time schedule (2) costs
// 1.5 GB and 0.6 ms; only 0 gains on the whole step (profiles/tri_rowfused_z_once_*.txt)
constexpr int RF_DEFAULT_TOUCH = 0;

struct TriRowArgs {
    const float* z; long long zb, zs, zl;                    // element (b, s, l, c) at z + b zb + s zs + l zl + c
    const char* wp; const float* csum; const float* bias;    // AbxTriRowPack
    float cs, inv_cs, eps;                                   // 2^-(a_exp + b_exp), its inverse, LayerNorm eps
    int order;
    int touch;                                               // the issuing wave's touches of z: 0 none, 1 the next slot's whole row at the start of
                                                             // phase A, 2 per k-group just ahead of the walk (tri_row_touch.h)
};

__global__ __launch_bounds__(TRI_THREADS) void tri_attn8_rowfused_kernel(const AbxTriAttn a, const TriRowArgs p) {
    constexpr int PLN = RF_PLN;
    constexpr int NCW = TRI_THREADS / 64 - 1;               // computing waves; the last wave issues the weight DMA
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* lds = reinterpret_cast<char*>(smem);
    float* Msb = reinterpret_cast<float*>(lds + RF_OFF_MSB);
    char* ring = lds + RF_OFF_RING;
    float* cst = reinterpret_cast<float*>(lds + RF_OFF_CONST);
    const int L = a.L;
    const ClockProbe probe(a.clock_probe);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ---- the slots of this workgroup: XCD x = blockIdx & 7 owns the rows (order 0) / the (b, h) pairs (order 1) x, x + 8, ...
    const int xcd = blockIdx.x & 7, wg = blockIdx.x >> 3, NW = gridDim.x >> 3;
    // (32-bit: the dispatch keeps B S H below 2^31; 64-bit divisions are ~80 vector instructions each)
    const unsigned nunit = p.order == 0 ? (unsigned)a.B * (unsigned)a.S : (unsigned)a.B * (unsigned)a.H;
    const unsigned per_unit = p.order == 0 ? (unsigned)a.H : (unsigned)a.S;
    const unsigned nslots = (nunit + 7 - xcd) / 8 * per_unit;                   // slots of this XCD (every one is valid)
    const int nmine = (unsigned)wg < nslots ? (int)((nslots - wg + NW - 1) / NW) : 0;       // slots wg, wg + NW, ... of them
    auto decode = [&](int i, Tri8Row& r) __attribute__((always_inline)) {
        const unsigned slot = (unsigned)wg + (unsigned)i * (unsigned)NW;
        const unsigned unit = slot / per_unit * 8 + xcd;
        const int sub = (int)(slot % per_unit);
        if (p.order == 0) { r.b = (int)(unit / (unsigned)a.S); r.s = (int)(unit % (unsigned)a.S); r.h = sub; }
        else { r.b = (int)(unit / (unsigned)a.H); r.h = (int)(unit % (unsigned)a.H); r.s = sub; }
        r.b = __builtin_amdgcn_readfirstlane(r.b);
        r.h = __builtin_amdgcn_readfirstlane(r.h);
        r.s = __builtin_amdgcn_readfirstlane(r.s);
        r.part = 0;
        r.base = 0;                                              // (no q | k | v rows in memory, no gate)
        r.km = a.keymask ? a.keymask + (long long)r.b * a.km_sb : nullptr;
        r.biasb = a.bias + (long long)r.b * a.bias_sb + (long long)r.h * a.bias_sh;
    };

    if (wave == NCW) {
        // ================= issuing wave ===================================================================================================
        // The 15 stages of a slot's head in three groups: G0 = stages 0 - 2 -> the ring (requested while the computing waves are in phase A
        // of the previous slot), G1 = 3 - 8 and G2 = 9 - 14 -> the plane region, which is empty between barrier (a) of a slot - every wave
        // has left phase A of the previous one - and its tile epilogues.  Barriers of a slot: (a) G0 landed, (b) G1, the key clamps and
        // the column constants landed (G2 in flight), (c) G2 landed, (d) every wave has read its last weight fragment (the epilogues may write K / V over
        // them), (e) K / V complete.  Inside a group the waves run free.
        __builtin_amdgcn_s_setprio(3);
        Tri8Row r;
        auto dma = [&](int hd, int s0, auto ns_, char* dst) __attribute__((always_inline)) {
            constexpr int NI = decltype(ns_)::value * (RF_STAGE / 1024);
            const char* src = p.wp + (long long)hd * RF_HEAD_BYTES + s0 * RF_STAGE + lane * 16;
#pragma unroll 8
            for (int i = 0; i < NI; ++i) glds16(src + i * 1024, dst + i * 1024);
        };
        // touch == 2: the RFT_N loads of k-group g of a row, one per 128-byte line.  They are inline assembly into ONE register that nothing
        // reads: the compiler places no wait for them (a wait of its own between the DMA instructions would drain the queue), and the
        // register stays allocated up to barrier (a), whose vmcnt(0) retires the last of them.
        const bool jit = p.touch == 2;
        unsigned tv = 0;
        auto touch_kg = [&](const float* zr, int g) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < RFT_N; ++i) {
                const float* q = zr + rf_touch_offset(L, p.zl, g, lane, i);
                asm volatile("global_load_dword %0, %1, off" : "+v"(tv) : "v"(q) : "memory");
            }
        };
        if (nmine > 0) {
            decode(0, r);
            dma(r.h, 0, std::integral_constant<int, RF_G0>{}, ring);
        }
        for (int it = 0; it < nmine; ++it) {
            decode(it, r);
            const float* zcur = p.z + (long long)r.b * p.zb + (long long)r.s * p.zs;
            // key clamps of the slot, applied as logit = min(logit, clamp): +inf valid, finfo.min masked, -inf beyond L (tri_attn8_kernel), and
            // the column constants of its head (read by the tile epilogues).  Their loads are issued HERE, in front of barrier (a) - this wave
            // idles there through phase A of the previous slot - and are UNCONDITIONAL (no key mask: the same number of loads from the
            // column sums, results dropped): behind barrier (a) this wave's vector-memory queue holds the 96 DMA instructions and nothing
            // else, so the counted waits below are exact whatever the descriptor holds.
            float kmv[6], csv[3], biv[3];
            {
                const float* kmp = r.km ? r.km : p.csum;
                const int kmax = r.km ? L - 1 : RF_TILES * 32 - 1;
#pragma unroll
                for (int j = 0; j < 6; ++j) kmv[j] = kmp[min(lane + 64 * j, kmax)];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int t = min(lane + 64 * j, RF_TILES * 32 - 1);
                    csv[j] = p.csum[r.h * (RF_TILES * 32) + t];
                    biv[j] = p.bias[r.h * (RF_TILES * 32) + t];
                }
            }
            // (a): G0 (requested a phase ago), the touches and the loads above have landed; the values pass through the statement, so the
            // compiler has no wait of its own to place between the DMA instructions below
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier"
                         : "+v"(kmv[0]), "+v"(kmv[1]), "+v"(kmv[2]), "+v"(kmv[3]), "+v"(kmv[4]), "+v"(kmv[5]), "+v"(csv[0]), "+v"(csv[1]), "+v"(csv[2]),
                           "+v"(biv[0]), "+v"(biv[1]), "+v"(biv[2]), "+v"(tv)
                         :
                         : "memory");
            if (jit) {
                // G1, the touches of k-group 1 (the computing waves walk k-group 0 from here on), G2
                dma(r.h, RF_G0, std::integral_constant<int, (RF_SPS - RF_G0) / 2>{}, lds);
                touch_kg(zcur, 1);
                dma(r.h, RF_G0 + (RF_SPS - RF_G0) / 2, std::integral_constant<int, (RF_SPS - RF_G0) / 2>{}, lds + (RF_SPS - RF_G0) / 2 * RF_STAGE);
            } else {
                dma(r.h, RF_G0, std::integral_constant<int, RF_SPS - RF_G0>{}, lds);
            }
            const bool has_km = r.km != nullptr;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int t = lane + 64 * j;
                Msb[t] = (t < L) ? ((!has_km || kmv[j] != 0.f) ? INFINITY : ABX_NEG_MAX) : -INFINITY;
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int t = lane + 64 * j;
                if (t < RF_TILES * 32) {
                    cst[t] = csv[j];
                    cst[RF_TILES * 32 + t] = biv[j];
                }
            }
            // (b): G1 = the first 48 of the 96 DMA instructions has landed (results return in issue order; the 48 of G2 stay in flight)
            // (c): G2 has landed.  touch == 2: the touches of k-group 2 go out behind (b), while the computing waves walk k-group 1
            if (jit) {
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(RF_VM_B_JIT) : "memory");
                touch_kg(zcur, 2);
                asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(RF_VM_C_JIT) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(RF_VM_B) : "memory");
                asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(RF_VM_C) : "memory");
            }
            asm volatile("s_barrier" ::: "memory");                                            // (d)
            asm volatile("s_barrier" ::: "memory");                                            // (e)
            // while the computing waves are in phase A: G0 of the NEXT slot, and a touch of its z row (one load per 128-byte line), so that its
            // projection starts from the L2 instead of waiting out an HBM round trip in front of every wave's first k-tile: the whole row
            // (touch == 1: 270 KB that have to survive phase A in the L2) or the lines of k-group 0 alone (touch == 2)
            if (it + 1 < nmine) {
                decode(it + 1, r);
                dma(r.h, 0, std::integral_constant<int, RF_G0>{}, ring);
                const float* zr = p.z + (long long)r.b * p.zb + (long long)r.s * p.zs;
                if (jit) {
                    touch_kg(zr, 0);
                } else if (p.touch == 1) {
                    unsigned x = 0;
                    for (int l = lane; l < L; l += 64) {
                        const float* zq = zr + (long long)l * p.zl;
#pragma unroll
                        for (int j = 0; j < 6; ++j) x ^= __builtin_bit_cast(unsigned, zq[j * 32]);
                    }
                    asm volatile("" ::"v"(x));
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(tv) : : "memory");
        probe.finish();
        return;
    }

    // ================= computing waves ======================================================================================
    const float qscale = a.scale * LOG2E * 8.0f;                          // (the scales of tri_attn8_kernel)
    const int nqt = (L + 15) / 16;
    const int qtA = 2 * wave;
    const bool has_tile = qtA < nqt;                                      // == the wave has rows to project (32 w < L)
    const float invK = 1.0f / (float)(RF_NK * 16);
    bool any_masked = false;
    int b_masked = -1;
    Tri8Row cur;
    for (int it = 0; it < nmine; ++it) {
        decode(it, cur);
        if (cur.b != b_masked) {                                // wave-uniform: does this sample mask any key?
            any_masked = false;
            if (cur.km) {
                for (int j = lane; j < L; j += 64) any_masked |= cur.km[j] == 0.f;
                any_masked = __any(any_masked);
            }
            b_masked = cur.b;
        }
        f16x8 qf[2][4];
        bool badp = false;
        // (the per-lane constants of a phase are recomputed per slot behind an opaque lane id: as invariants of the whole kernel they are held
        // across BOTH phases and spill - the producer of tri_attn8_kernel does the same)
        int ln = threadIdx.x & 63;
        asm volatile("" : "+v"(ln));
        const int hh = ln >> 5, pr = ln & 31;                               // projection lane = (position of the wave's 32, k half / channel half)
        const int foff = pr * 32 + ((hh ^ ((pr >> 3) & 1)) << 4);           // weight fragment inside a (k-tile, plane) image of the ring
        float m2048 = -2048.0f, c16 = 16.0f;
        asm volatile("" : "+v"(m2048), "+v"(c16));
        // ---- phase P.  Stage (kg, t) = k-tiles 4 kg .. 4 kg + 3 of column tile t: the wave holds the pieces of four k-tiles (32 registers) and
        // the accumulators of all five column tiles (80); every output element still sums its k-tiles in ascending order.
        // Pieces and statistics: as_conv_ktile / as_conv_finish of gemm_as.hip, k-tiles in order.
        f32x16 acc[RF_TILES];
#pragma unroll
        for (int t = 0; t < RF_TILES; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
        // (positions beyond the row: the last one again - keys clamped to -inf, queries never stored)
        const float* zp = p.z + (long long)cur.b * p.zb + (long long)cur.s * p.zs + rf_walk_base(L, p.zl, wave, pr, hh);
        float lshift = 0.f;
        f32x2 ls2 = {0.f, 0.f}, lq2 = {0.f, 0.f};
        static_for<0, 3>([&](auto kg_) __attribute__((always_inline)) {
            constexpr int kg = decltype(kg_)::value;
            u32x4 a0[4], a1[4];
            if (has_tile) {
                f32x4 lo[4], hi[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    lo[kk] = *reinterpret_cast<const f32x4*>(zp + rf_walk_ktile(4 * kg + kk));
                    hi[kk] = *reinterpret_cast<const f32x4*>(zp + rf_walk_ktile(4 * kg + kk) + 4);
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    float xv[8];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { xv[e] = lo[kk][e]; xv[4 + e] = hi[kk][e]; }
                    if (kg == 0 && kk == 0) lshift = __shfl(xv[0], pr, 64);      // the row's first element
                    const f32x2 sh2 = {lshift, lshift};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        f32x2 xp = {xv[2 * e], xv[2 * e + 1]};
                        xp -= sh2;
                        ls2 += xp;
                        lq2 = __builtin_elementwise_fma(xp, xp, lq2);
                        xv[2 * e] = xp[0];
                        xv[2 * e + 1] = xp[1];
                    }
                    unsigned q0[4], q1[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) split2h_mix(xv[2 * e], xv[2 * e + 1], m2048, q0[e], q1[e]);
                    a0[kk] = u32x4{q0[0], q0[1], q0[2], q0[3]};
                    a1[kk] = u32x4{q1[0], q1[1], q1[2], q1[3]};
                }
            }
            static_for<0, RF_TILES>([&](auto t_) __attribute__((always_inline)) {
                constexpr int t = decltype(t_)::value;
                constexpr int n = kg * RF_TILES + t;                                  // stage of the slot
                // (the issuing wave's barriers (a), (b), (c): the stage's group has landed)
                if constexpr (n == 0 || n == RF_G0 || n == RF_G0 + (RF_SPS - RF_G0) / 2) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if (has_tile) {
                    const char* ws = (n < RF_G0 ? ring + n * RF_STAGE : lds + (n - RF_G0) * RF_STAGE) + foff;
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const u32x4 w0 = *reinterpret_cast<const u32x4*>(ws + kk * 2048);
                        const u32x4 w1 = *reinterpret_cast<const u32x4*>(ws + kk * 2048 + 1024);
                        const u32x4 w2 = f16x8_lo(w0);
                        // a1 p2, a0 p1, a0 p0 (smallest first), from a zero accumulator
                        acc[t] = mfma_split(w2, a1[kk], acc[t]);
                        acc[t] = mfma_split(w1, a0[kk], acc[t]);
                        acc[t] = mfma_split(w0, a0[kk], acc[t]);
                    }
                }
            });
        });
        float dm = 0.f, rs = 0.f;
        {
            const float ls = ls2[0] + ls2[1], lqs = lq2[0] + lq2[1];
            const float sm = ls + __shfl_xor(ls, 32, 64), sq = lqs + __shfl_xor(lqs, 32, 64);
            dm = sm * invK;
            rs = (1.0f / sqrtf(fmaxf(sq * invK - dm * dm, 0.f) + p.eps)) * p.cs;
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // (d) every wave has read its last weight fragment out of the plane region
        // ---- the five column tiles: k 0..31 | k 32..47, v 0..15 | v 16..47 | q (16 hh ..) | q 32..47 (both halves)
        const float* cst_l = cst + 4 * hh;
        char* kdst = lds + (32 * wave + pr) * RST + hh * 16;            // (plane p1: + PLN; V planes: + 2 PLN)
        static_for<0, RF_TILES>([&](auto t_) __attribute__((always_inline)) {
            constexpr int t = decltype(t_)::value;
            if (has_tile) {
                // folded-LayerNorm epilogue (gemm_as plain_slice): register 4 i + c = packed column 8 i + 4 hh + c of the tile
                float x[16];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 cs4 = *reinterpret_cast<const f32x4*>(cst_l + t * 32 + 8 * i);
                    const f32x4 bi4 = *reinterpret_cast<const f32x4*>(cst_l + RF_TILES * 32 + t * 32 + 8 * i);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float csump = cs4[c] * p.inv_cs;
                        const float v = rs * (acc[t][4 * i + c] - dm * csump);
                        x[4 * i + c] = v + bi4[c];
                    }
                    badp |= __builtin_amdgcn_classf((x[4 * i] + x[4 * i + 1]) + (x[4 * i + 2] + x[4 * i + 3]), 0x207);
                }
                if constexpr (t < 3) {
                    // registers 0..7 / 8..15: 8 consecutive channels each -> planes p0, p1 of 16 x value (the producer's split2b_mix)
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        // tile 0: K 8 hh, K 16 + 8 hh; tile 1: K 32 + 8 hh, V 8 hh; tile 2: V 16 + 8 hh, V 32 + 8 hh
                        constexpr int TAB[3][2] = {{0, 32}, {64, 2 * PLN}, {2 * PLN + 32, 2 * PLN + 64}};
                        unsigned w0[4], w1[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) split2b_mix(x[8 * half + 2 * e], x[8 * half + 2 * e + 1], c16, w0[e], w1[e]);
                        char* d = kdst + TAB[t][half];
                        *reinterpret_cast<u32x4*>(d) = u32x4{w0[0], w0[1], w0[2], w0[3]};
                        *reinterpret_cast<u32x4*>(d + PLN) = u32x4{w1[0], w1[1], w1[2], w1[3]};
                    }
                } else {
                    // q: lanes l and l ^ 16 hold the positions lq and 16 + lq of the same channels; query tile X = 0 takes registers 0..7 of the
                    // even 16-lane row, X = 1 registers 8..15 of the odd one (v_permlane16_swap: odd rows of the first <-> even rows of the second)
                    float qv[2][8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(x[e]), __float_as_uint(x[8 + e]), false, false);
                        qv[0][e] = __uint_as_float(sw[0]);
                        qv[1][e] = __uint_as_float(sw[1]);
                    }
#pragma unroll
                    for (int X = 0; X < 2; ++X) {
                        unsigned p0[4], p1[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) split2h_ns(qv[X][2 * e] * qscale, qv[X][2 * e + 1] * qscale, p0[e], p1[e]);
                        if constexpr (t == 3) {
                            qf[X][0] = __builtin_bit_cast(f16x8, u32x4{p0[0], p0[1], p0[2], p0[3]});
                            qf[X][1] = __builtin_bit_cast(f16x8, u32x4{p1[0], p1[1], p1[2], p1[3]});
                        } else {
                            qf[X][2] = __builtin_bit_cast(f16x8, u32x4{p0[0], p0[1], p0[2], p0[3]});
                            qf[X][3] = hh == 0 ? __builtin_bit_cast(f16x8, u32x4{p1[0], p1[1], p1[2], p1[3]}) : __builtin_bit_cast(f16x8, u32x4{0u, 0u, 0u, 0u});
                        }
                    }
                }
            }
        });
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // (e) the K / V planes and the clamps of the row are complete
        // ---- phase A
        int cc = 0;
        int la = threadIdx.x & 63;
        asm volatile("" : "+v"(la));
        const int lqa = la & 15, ga = la >> 4;
        const int koff0 = lqa * RST + ga * 16;
        const int koffc = lqa * RST + (ga >> 1) * PLN + 64 + (ga & 1) * 16;
        const int voff = (4 * ga + (lqa >> 2)) * RST + (lqa & 3) * 8;
        unsigned boff[2];
#pragma unroll
        for (int X = 0; X < 2; ++X) {
            const int qrow = min((qtA + X) * 16 + lqa, L - 1);     // beyond the row: the last query row again (never stored)
            boff[X] = (unsigned)(((long long)qrow * a.bias_sq + ga * 4) * 4);
        }
        if (a.range_flag && __any(badp) && la == 0) atomicOr(a.range_flag, a.range_tag);
        tri8_row_compute<RF_LK, true, false>(a, cur, lds, Msb, cc, 1, qf, boff, any_masked, has_tile, qtA, nqt, la, koff0, koffc, voff,
                                             []() __attribute__((always_inline)) {});
    }
    probe.finish();
}

// head-major image of the q | k | v planes for tri_attn8_rowfused_kernel: per head 3 groups of 4 k-tiles x 5 column tiles, each (group, tile) the
// 8 KB ring stage [k-tile][plane][column 32][16] in the bank-swizzled fragment order; packed column m of a tile -> source column:
//   tiles 0 - 2 (k 0..31 | k 32..47, v 0..15 | v 16..47): channel 16 (i >> 1) + 8 hh + 4 (i & 1) + c of the tile's 32 (m = 8 i + 4 hh + c)
//   tile 3: q channel 16 hh + 4 i + c; tile 4: q channel 32 + 4 i + c for both hh
__device__ __forceinline__ int rf_source_col(int h, int t, int m) {
    const int i = m >> 3, hh = (m >> 2) & 1, c = m & 3;
    const int kv = 16 * (i >> 1) + 8 * hh + 4 * (i & 1) + c;
    if (t == 0) return 192 + 48 * h + kv;
    if (t == 1) return kv < 16 ? 192 + 48 * h + 32 + kv : 384 + 48 * h + (kv - 16);
    if (t == 2) return 384 + 48 * h + 16 + kv;
    if (t == 3) return 48 * h + 16 * hh + 4 * i + c;
    return 48 * h + 32 + 4 * i + c;
}
__global__ void tri_rowpack_kernel(const unsigned short* __restrict__ planes, const float* __restrict__ csum, const float* __restrict__ bias,
                                   int N, int H, unsigned short* __restrict__ out, float* __restrict__ csum_h, float* __restrict__ bias_h) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;      // one thread per (head, tile, packed column, k-tile, plane, k half)
    const int total = H * RF_TILES * 32 * RF_NK * 2 * 2;
    if (idx >= total) return;
    int r = idx;
    const int half = r & 1; r >>= 1;
    const int plane = r & 1; r >>= 1;
    const int kt = r % RF_NK; r /= RF_NK;
    const int m = r & 31; r >>= 5;
    const int t = r % RF_TILES, h = r / RF_TILES;
    const int n = rf_source_col(h, t, m);
    const unsigned short* src = planes + (((long long)kt * 2 + plane) * N + n) * 16 + half * 8;
    unsigned short* dst = out + ((long long)h * RF_HEAD_BYTES + ((kt / 4) * RF_TILES + t) * RF_STAGE + (kt % 4) * 2048 + plane * 1024 + m * 32 +
                                 ((half ^ ((m >> 3) & 1)) << 4)) / 2;
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e] = src[e];
    if (kt == 0 && plane == 0 && half == 0) {
        csum_h[(h * RF_TILES + t) * 32 + m] = csum[n];
        bias_h[(h * RF_TILES + t) * 32 + m] = bias[n];
    }
}

// ---- sequence attention with pair bias (seqformer.py:314-356): 32 heads x 17 channels, bias (b, h, q, k) ---------------------------
// The bias stream (L^2 floats per (b, h): 1.6 GB per launch at B = 100, L = 352) is the only real traffic, so the kernel is laid
// out around reading it coalesced: a wave takes 4 queries at a time and its LANES ARE KEYS (key = lane + 64 m), each bias row is
// read as contiguous 256-byte segments.  K and V of the (b, h) pair sit in LDS as [key][20] (17 channels + zero pad: 16-byte
// reads); the 4 x 17 query values are wave-uniform.
//   logits  lane: 17 FMAs per (query, key) against its K row (read once for the 4 queries), + bias, key mask
//   softmax per query over lanes (wave max / sum, base 2)
//   PV      the weights go through a wave-private LDS strip and the lanes regroup as (query, 4 channels, key quarter): one
//           16-byte V read + one weight read per 4 FMAs; the 17th channel as (query, key sixteenth); shuffle folds, fixed order
// NT threads share the K / V of one (b, h) pair: 16 waves (4 per SIMD, hiding the LDS / shuffle latencies) while the weight strips fit
template <int NK, int NT>
__global__ __launch_bounds__(NT) void seq_attn2_kernel(const float* __restrict__ qkv, const float* __restrict__ bias,
                                                        const float* __restrict__ keymask, const float* __restrict__ gate,
                                                        float* __restrict__ out, int L, int H, float scale, int qblk) {
    constexpr int D = 17, DP = 20, QW = 4, LP = NK * 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;                       // [L][DP]
    float* Vs = smem + (size_t)L * DP;      // [L][DP]
    float* pw = Vs + (size_t)L * DP;        // [waves][QW][LP]
    const int h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long ld = (long long)H * 3 * D;
    const float* rowb = qkv + (long long)b * L * ld + (long long)h * 3 * D;
    for (int idx = tid; idx < L * DP; idx += NT) {
        const int key = idx / DP, d = idx - key * DP;
        Ks[idx] = d < D ? rowb[(long long)key * ld + D + d] : 0.f;
        Vs[idx] = d < D ? rowb[(long long)key * ld + 2 * D + d] : 0.f;
    }
    __syncthreads();
    const float qs = scale * LOG2E;
    const float* km = keymask ? keymask + (long long)b * L : nullptr;
    // per-lane key clamps: +inf valid, finfo.min masked (the reference REPLACES the logit: every finite logit is >= finfo.min),
    // -inf beyond L
    float clampv[NK];
#pragma unroll
    for (int m = 0; m < NK; ++m) {
        const int k = lane + 64 * m;
        clampv[m] = k < L ? ((!km || km[k] != 0.f) ? INFINITY : ABX_NEG_MAX) : -INFINITY;
    }
    float* pww = pw + (size_t)wave * QW * LP;
    const int q_end = min((int)(blockIdx.x + 1) * qblk, L);
    for (int qb = blockIdx.x * qblk + wave * QW; qb < q_end; qb += (NT / 64) * QW) {
        // ---- bias rows of the 4 queries (coalesced), issued first
        float bz[QW][NK];
#pragma unroll
        for (int qq = 0; qq < QW; ++qq) {
            const float* bp = bias + (((long long)b * H + h) * L + min(qb + qq, L - 1)) * L;
#pragma unroll
            for (int m = 0; m < NK; ++m) bz[qq][m] = bp[min(lane + 64 * m, L - 1)];
        }
        // ---- logits (base 2)
        float sc[QW][NK];
#pragma unroll
        for (int m = 0; m < NK; ++m) {
            const float* kr = Ks + (size_t)min(lane + 64 * m, L - 1) * DP;
            f32x4 kv[DP / 4];
#pragma unroll
            for (int c = 0; c < DP / 4; ++c) kv[c] = *reinterpret_cast<const f32x4*>(kr + c * 4);
#pragma unroll
            for (int qq = 0; qq < QW; ++qq) {
                const float* qp = rowb + (long long)min(qb + qq, L - 1) * ld;          // wave-uniform
                float acc = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) acc = fmaf(qp[d] * qs, kv[d >> 2][d & 3], acc);
                sc[qq][m] = fminf(fmaf(bz[qq][m], LOG2E, acc), clampv[m]);
            }
        }
        // ---- softmax over the keys (lanes x NK), the 4 queries interleaved
        float inv[QW];
#pragma unroll
        for (int qq = 0; qq < QW; ++qq) {
            float mx = sc[qq][0];
#pragma unroll
            for (int m = 1; m < NK; ++m) mx = fmaxf(mx, sc[qq][m]);
            mx = wave_max(mx);
            float sm = 0.f;
#pragma unroll
            for (int m = 0; m < NK; ++m) {
                const float pv = __builtin_amdgcn_exp2f(sc[qq][m] - mx);
                sc[qq][m] = pv;
                sm += pv;
            }
            inv[qq] = 1.0f / wave_sum(sm);
        }
#pragma unroll
        for (int qq = 0; qq < QW; ++qq)
#pragma unroll
            for (int m = 0; m < NK; ++m) pww[qq * LP + lane + 64 * m] = sc[qq][m];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- PV, channels 0..15: lane = (query, channel quad, key quarter)
        const int qq = lane >> 4, qi = qb + qq;
        const float myinv = qq == 0 ? inv[0] : (qq == 1 ? inv[1] : (qq == 2 ? inv[2] : inv[3]));
        const float* pr = pww + qq * LP;
        const long long orow = ((long long)b * L + min(qi, L - 1)) * H * D + (long long)h * D;
        {
            const int dg = (lane >> 2) & 3, kg = lane & 3;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int k = kg; k < L; k += 4) {
                const float w = pr[k];
                const f32x4 v4 = *reinterpret_cast<const f32x4*>(Vs + (size_t)k * DP + dg * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = fmaf(w, v4[c], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[c] += __shfl_xor(acc[c], 1, 64);
                acc[c] += __shfl_xor(acc[c], 2, 64);
            }
            if (kg == 0 && qi < q_end) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float v = acc[c] * myinv;
                    if (gate) v *= sigmoidf_(gate[orow + dg * 4 + c]);
                    out[orow + dg * 4 + c] = v;
                }
            }
        }
        // ---- channel 16: lane = (query, key sixteenth)
        {
            const int kg = lane & 15;
            float acc = 0.f;
#pragma unroll 4
            for (int k = kg; k < L; k += 16) acc = fmaf(pr[k], Vs[(size_t)k * DP + 16], acc);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) acc += __shfl_xor(acc, o, 64);
            if (kg == 0 && qi < q_end) {
                float v = acc * myinv;
                if (gate) v *= sigmoidf_(gate[orow + 16]);
                out[orow + 16] = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

// abx_tri_attn_fwd (plan == nullptr) / abx_tri_attn_plan: the kernel is launched or named where it is chosen
static int tri_attn_run(const AbxTriAttn* ap, hipStream_t st, AbxPlan* plan) {
    ABX_REQUIRE(ap != nullptr, "abx_tri_attn_fwd: null descriptor");
    const AbxTriAttn a = *ap;
    ABX_REQUIRE(a.q && a.k && a.v && a.out, "abx_tri_attn_fwd: null operand");
    ABX_REQUIRE(a.D == TD, "abx_tri_attn_fwd: head dim must be 48");
    ABX_REQUIRE(a.B > 0 && a.S > 0 && a.L > 0 && a.H > 0, "abx_tri_attn_fwd: empty problem");
    ABX_REQUIRE(a.S <= 65535 && a.B <= 65535, "abx_tri_attn_fwd: grid too large");
    ABX_REQUIRE((a.sb % 4 == 0) && (a.ss % 4 == 0) && (a.sl % 4 == 0) && (a.ob % 4 == 0) && (a.os % 4 == 0) && (a.ol % 4 == 0),
                "abx_tri_attn_fwd: strides must be multiples of 4 floats");
    ABX_REQUIRE(al16(a.q) && al16(a.k) && al16(a.v) && al16(a.out) && (!a.gate || al16(a.gate)),
                "abx_tri_attn_fwd: pointers must be 16-byte aligned");
    ABX_REQUIRE(!a.kv_planes || !a.exact, "abx_tri_attn_fwd: kv_planes goes with the split-f16 kernel (exact = 0)");
    if (!a.exact) {
        // split-f16 kernel: K / V staged in (double-buffered) key chunks, a wave keeps the online-softmax state of up to MAXQ query tiles
        // A workgroup carries 2 query-tile slots per wave: 24 tiles with 12 computing waves, 22 with 11 + the producer wave.  Rows with
        // more tiles are dealt to q_parts workgroups of (almost) equal share; the producer variant whenever the share fits its 22.
        // (Every query's arithmetic is the same in all variants: results are bit-identical.)  tune bit 0: never the producer wave.
        AbxTriAttn aa = a;
        const int nqt = (a.L + 15) / 16, nw = TRI_THREADS / 64;
        // tri_attn8_kernel: 11 computing waves x 2 query tiles walked together (its producer addresses a (b, s) slab of K / V with 32-bit
        // byte offsets and a 24-bit row stride; any other layout takes tri_attn4)
        const bool paired = !(a.tune & 4) && a.sl * 4 < (1LL << 24) && (long long)a.L * a.sl * 4 < (1LL << 32);
        ABX_REQUIRE(!a.kv_planes || paired, "abx_tri_attn_fwd: kv_planes (k | v as operand images) is served by tri_attn8_kernel only (tune bit 2 off, "
                                            "key stride below 2^24 bytes)");
        aa.q_parts = paired ? (nqt + 2 * (nw - 1) - 1) / (2 * (nw - 1)) : (nqt + 2 * nw - 1) / (2 * nw);
        const int tpp = (nqt + aa.q_parts - 1) / aa.q_parts;
        const bool prod = tpp <= 2 * (nw - 1) && !(a.tune & 1);
        aa.row_groups = ((long long)a.B * a.H) % 8 == 0 ? 1 : 2;
        const long long nvp8 = ((long long)a.B * a.H * aa.row_groups + 7) / 8 * 8, rows_g = (a.S + aa.row_groups - 1) / aa.row_groups;
        ABX_REQUIRE(nvp8 * rows_g * aa.q_parts < (1LL << 31), "abx_tri_attn_fwd: grid too large");
        // tri_attn4: one workgroup per (b, h, row, part) slot; tri_attn8: persistent, one workgroup per CU (8 XCDs x CUs / 8), each
        // walking the slots of its XCD with a stride of the workgroups per XCD
        static int n_cu = 0;
        if (paired && n_cu == 0 && !plan) {
            int dev = 0;
            hipDeviceProp_t prop;
            if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
                abx_set_error("abx_tri_attn_fwd: hipGetDeviceProperties failed");
                return ABX_ERR_ARG;
            }
            n_cu = prop.multiProcessorCount > 8 ? prop.multiProcessorCount / 8 * 8 : 8;
        }
        const long long slots_xcd = nvp8 / 8 * rows_g * aa.q_parts;
        const unsigned wg_xcd = paired ? (unsigned)std::min<long long>(n_cu / 8, slots_xcd) : 0;
        const dim3 grid(paired ? 8 * wg_xcd : (unsigned)(nvp8 * rows_g * aa.q_parts)), block(TRI_THREADS);
        auto lds_of = [](int kc) { return (size_t)2 * (4 * kc * RST + kc * sizeof(float)); };      // double-buffered key chunks
#define TRI8_LAUNCH(KC, BVEC)                                                                                                                    \
    ABX_LAUNCH(plan, ("tri_attn8_kernel<%d, %d, %s>", KC, TRI_THREADS, ABX_BOOL(BVEC)), "abx_tri_attn_fwd", (&tri_attn8_kernel<KC, TRI_THREADS, BVEC>), \
               (int)lds_of(KC), grid, block, lds_of(KC), st, aa)
#define TRI4_LAUNCH(KC, PROD)                                                                                                                    \
    ABX_LAUNCH(plan, ("tri_attn4_kernel<2, %d, true, %d, %s>", KC, TRI_THREADS, ABX_BOOL(PROD)), "abx_tri_attn_fwd",                              \
               (&tri_attn4_kernel<2, KC, true, TRI_THREADS, PROD>), (int)lds_of(KC), grid, block, lds_of(KC), st, aa)
        if (paired) {
            const float* bb = a.bias;
            const bool bvec = bb && a.bias_sk == 1 && a.bias_sq % 4 == 0 && a.bias_sq >= 4 && a.bias_sb % 4 == 0 && a.bias_sh % 4 == 0 && al16(bb);
            // key chunks of 192 unless 128 gives the same number of chunks (then: less LDS to fill before the first tile, a less ragged
            // last chunk; L = 231: 2.52 vs 2.79 ms at 20 samples, L = 352: 21.2 vs 19.2 ms at 100).  tune bit 1 flips the choice.
            const bool kc128 = (((a.L + 127) / 128 == (a.L + 191) / 192) != ((a.tune & 2) != 0));
            if (kc128) return bvec ? TRI8_LAUNCH(128, true) : TRI8_LAUNCH(128, false);
            return bvec ? TRI8_LAUNCH(192, true) : TRI8_LAUNCH(192, false);
        }
        if (prod && (a.tune & 2)) return TRI4_LAUNCH(128, true);   // benchmarking
        if (prod) return TRI4_LAUNCH(192, true);
        return TRI4_LAUNCH(128, false);
#undef TRI8_LAUNCH
#undef TRI4_LAUNCH
    }
    // exact fp32 kernel: the whole row's K / V in LDS when it fits (L <= 389), key chunks of 320 otherwise (no length limit)
    auto lds_of_exact = [](int kc) { return ((((size_t)kc * LDK + 3) & ~(size_t)3) + (size_t)kc * LDV + (size_t)((kc + 63) / 64) * 64 + 4) * sizeof(float); };
    const int kc = lds_of_exact(a.L) <= 160 * 1024 ? a.L : 320;      // (chunks start at multiples of 64: aligned bias loads)
    const size_t lds = lds_of_exact(kc);
    ABX_REQUIRE(lds <= 160 * 1024, "abx_tri_attn_fwd: internal: exact-kernel LDS layout");
    return ABX_LAUNCH_LIT(plan, "abx_tri_attn_fwd", &tri_attn_kernel, 160 * 1024, dim3(a.H, a.S, a.B), dim3(TRI_THREADS), lds, st, a, kc);
}

extern "C" int abx_tri_attn_fwd(const AbxTriAttn* ap, hipStream_t st) { return tri_attn_run(ap, st, nullptr); }

// abx_seq_attn_fwd (plan == nullptr) / abx_seq_attn_plan: the kernel is launched or named where it is chosen; qblk_out (nullable) receives
// the query rows per workgroup of that launch
static int seq_attn_run(const float* qkv, const float* bias, const float* keymask, const float* gate, float* out, int B, int L, int H, int D,
                        float scale, hipStream_t st, AbxPlan* plan, int* qblk_out) {
    ABX_REQUIRE(qkv && bias && out && B > 0 && L > 0 && H > 0, "abx_seq_attn_fwd: bad args");
    ABX_REQUIRE(D == 17, "abx_seq_attn_fwd: head dim must be 17 (544 / 32)");
    ABX_REQUIRE(H <= 65535 && B <= 65535, "abx_seq_attn_fwd: grid too large");
    const int nk = (L + 63) / 64;
    ABX_REQUIRE(nk <= 12, "abx_seq_attn_fwd: L too large (L <= 716)");
    const int nkt = nk <= 2 ? 2 : (nk <= 4 ? 4 : (nk <= 6 ? 6 : (nk <= 8 ? 8 : 12)));       // keys per lane of the instantiation
    const int nt = nkt <= 6 ? 1024 : (nkt <= 8 ? 512 : 256);
    // one workgroup per (b, h) (every wave passes over 4 queries at a time); long complexes split the queries
    const int nb = (L + 511) / 512;
    const int qblk = (((L + nb - 1) / nb) + 3) / 4 * 4;
    const size_t lds = ((size_t)2 * L * 20 + (size_t)(nt / 64) * 4 * nkt * 64) * sizeof(float);
    ABX_REQUIRE(lds <= 160 * 1024, "abx_seq_attn_fwd: L too large for the LDS-resident K / V (L <= 716)");
    if (qblk_out) *qblk_out = qblk;
    const dim3 grid((L + qblk - 1) / qblk, H, B), block(nt);
#define SEQ_LAUNCH(NK, NT)                                                                                                                      \
    ABX_LAUNCH_LIT(plan, "abx_seq_attn_fwd", (&seq_attn2_kernel<NK, NT>), 160 * 1024, grid, block, lds, st, qkv, bias, keymask, gate, out, L, H, \
                   scale, qblk)
    switch (nkt) {
        case 2: return SEQ_LAUNCH(2, 1024);
        case 4: return SEQ_LAUNCH(4, 1024);
        case 6: return SEQ_LAUNCH(6, 1024);
        case 8: return SEQ_LAUNCH(8, 512);
        default: return SEQ_LAUNCH(12, 256);
    }
#undef SEQ_LAUNCH
}

extern "C" int abx_seq_attn_fwd(const float* qkv, const float* bias, const float* keymask, const float* gate, float* out,
                                int B, int L, int H, int D, float scale, hipStream_t st) {
    return seq_attn_run(qkv, bias, keymask, gate, out, B, L, H, D, scale, st, nullptr, nullptr);
}

extern "C" int abx_seq_attn_plan(int L, char* name, int cap, int* qblk) {
    ABX_REQUIRE(name && cap > 0, "abx_seq_attn_plan: no room for the name");
    AbxPlan plan = {};
    // one sample of the model's 32 heads x 17 channels on stand-in operands that pass the null checks - an address is looked at, never followed
    alignas(16) static float stand_in[4] = {};
    if (int rc = seq_attn_run(stand_in, stand_in, nullptr, nullptr, stand_in, 1, L, 32, 17, 0.f, nullptr, &plan, qblk)) return rc;
    snprintf(name, (size_t)cap, "%s", plan.name);
    return ABX_OK;
}

// ---- row-fused triangle attention: pack, switch, entry ------------------------------------------------------------------------------
namespace {
inline long long rf_up(long long x) { return (x + 255) / 256 * 256; }
}  // namespace

extern "C" long long abx_tri_rowpack_bytes(void) { return rf_up(4LL * RF_HEAD_BYTES) + 2 * rf_up(4LL * RF_TILES * 32 * 4); }

extern "C" int abx_tri_rowpack(const AbxLinearPack* qkv, void* buf, AbxTriRowPack* out, hipStream_t st) {
    ABX_REQUIRE(qkv && buf && out, "abx_tri_rowpack: bad args");
    ABX_REQUIRE(qkv->K == RF_NK * 16 && qkv->N == 3 * 4 * TD && qkv->planes && qkv->csum && qkv->bias,
                "abx_tri_rowpack: qkv = LayerNorm-folded 192 -> 576 pack with planes");
    ABX_REQUIRE((reinterpret_cast<uintptr_t>(buf) & 255) == 0, "abx_tri_rowpack: buf must be 256-byte aligned");
    char* p = static_cast<char*>(buf);
    unsigned short* planes = reinterpret_cast<unsigned short*>(p); p += rf_up(4LL * RF_HEAD_BYTES);
    float* csum = reinterpret_cast<float*>(p); p += rf_up(4LL * RF_TILES * 32 * 4);
    float* bias = reinterpret_cast<float*>(p);
    const int total = 4 * RF_TILES * 32 * RF_NK * 2 * 2;
    hipLaunchKernelGGL(tri_rowpack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, qkv->planes, qkv->csum, qkv->bias, qkv->N, 4, planes, csum, bias);
    if (int rc = abx_check_launch("abx_tri_rowpack")) return rc;
    out->planes = planes;
    out->csum = csum;
    out->bias = bias;
    out->b_exp = qkv->b_exp;
    out->H = 4;
    return ABX_OK;
}

extern "C" int abx_tri_attn_rowfused_ok(int L) {
    // (the Python side asks this function instead of reading the variable itself)
    static const bool off = abx_env_on("ABX_NO_TRI_ROWFUSED");
    return (!off && L > 0 && L <= ABX_TRI_ROWFUSED_LMAX) ? 1 : 0;
}

extern "C" int abx_tri_row_touch(int v) {
    // ABX_TRI_ROW_TOUCH = 0 | 1 | 2, read once on the C side (A / B measurements); anything else: the default
    static std::atomic<int> cur{[] {
        const char* e = getenv("ABX_TRI_ROW_TOUCH");
        return (e && e[0] >= '0' && e[0] <= '2' && e[1] == 0) ? e[0] - '0' : RF_DEFAULT_TOUCH;
    }()};
    return (v >= 0 && v <= 2) ? cur.exchange(v) : cur.load();
}

// abx_tri_attn_rowfused_fwd (plan == nullptr) / abx_tri_attn_plan
static int tri_attn_rowfused_run(const AbxTriAttn* ap, const float* z, long long zb, long long zs, long long zl, const AbxTriRowPack* pk,
                                 int slot_order, hipStream_t st, AbxPlan* plan) {
    ABX_REQUIRE(ap != nullptr && z && pk, "abx_tri_attn_rowfused_fwd: null argument");
    AbxTriAttn a = *ap;
    ABX_REQUIRE(a.out && a.bias && pk->planes && pk->csum && pk->bias, "abx_tri_attn_rowfused_fwd: null operand");
    ABX_REQUIRE(a.D == TD && a.H == 4 && pk->H == 4, "abx_tri_attn_rowfused_fwd: 4 heads of 48 channels");
    ABX_REQUIRE(a.B > 0 && a.S > 0 && a.L > 0, "abx_tri_attn_rowfused_fwd: empty problem");
    ABX_REQUIRE(a.L <= ABX_TRI_ROWFUSED_LMAX, "abx_tri_attn_rowfused_fwd: L beyond ABX_TRI_ROWFUSED_LMAX (the two launches serve longer rows)");
    ABX_REQUIRE(!a.exact && !a.kv_planes && !a.gate, "abx_tri_attn_rowfused_fwd: split-f16 arithmetic, no gate, no operand images");
    ABX_REQUIRE(slot_order >= -1 && slot_order <= 1, "abx_tri_attn_rowfused_fwd: slot_order is -1, 0 or 1");
    ABX_REQUIRE((zb % 4 == 0) && (zs % 4 == 0) && (zl % 4 == 0) && (a.ob % 4 == 0) && (a.os % 4 == 0) && (a.ol % 4 == 0) && al16(z) && al16(a.out) &&
                    al16(pk->planes) && al16(pk->csum) && al16(pk->bias),
                "abx_tri_attn_rowfused_fwd: strides must be multiples of 4 floats, pointers 16-byte aligned");
    ABX_REQUIRE(a.bias_sk == 1 && a.bias_sq % 4 == 0 && a.bias_sq >= a.L && a.bias_sb % 4 == 0 && a.bias_sh % 4 == 0 && al16(a.bias) &&
                    (long long)a.L * a.bias_sq * 4 < (1LL << 31),
                "abx_tri_attn_rowfused_fwd: the bias must be key-contiguous rows padded to a multiple of 4 floats, 16-byte aligned");
    ABX_REQUIRE(pk->b_exp >= -100 && pk->b_exp <= 100, "abx_tri_attn_rowfused_fwd: plane exponent out of range");
    ABX_REQUIRE((long long)a.B * a.S * a.H < (1LL << 31), "abx_tri_attn_rowfused_fwd: grid too large");
    a.q = a.k = a.v = nullptr;
    a.q_parts = 1;
    a.row_groups = 1;
    TriRowArgs p;
    p.z = z; p.zb = zb; p.zs = zs; p.zl = zl;
    p.wp = reinterpret_cast<const char*>(pk->planes); p.csum = pk->csum; p.bias = pk->bias;
    p.cs = ldexpf(1.0f, -ABX_F16_A_EXP - pk->b_exp);
    p.inv_cs = ldexpf(1.0f, ABX_F16_A_EXP + pk->b_exp);
    p.eps = 1e-5f;
    p.order = slot_order < 0 ? RF_DEFAULT_ORDER : slot_order;
    p.touch = abx_tri_row_touch(-1);
    static int n_cu = 0;
    if (n_cu == 0 && !plan) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
            abx_set_error("abx_tri_attn_rowfused_fwd: hipGetDeviceProperties failed");
            return ABX_ERR_ARG;
        }
        n_cu = prop.multiProcessorCount > 8 ? prop.multiProcessorCount / 8 * 8 : 8;
    }
    const long long nunit = p.order == 0 ? (long long)a.B * a.S : (long long)a.B * a.H;
    const long long slots_xcd = (nunit + 7) / 8 * (p.order == 0 ? a.H : a.S);
    const unsigned wg_xcd = (unsigned)std::min<long long>(n_cu / 8, slots_xcd);
    return ABX_LAUNCH_LIT(plan, "abx_tri_attn_rowfused_fwd", &tri_attn8_rowfused_kernel, RF_LDS, dim3(8 * wg_xcd), dim3(TRI_THREADS), RF_LDS, st, a, p);
}

extern "C" int abx_tri_attn_rowfused_fwd(const AbxTriAttn* ap, const float* z, long long zb, long long zs, long long zl, const AbxTriRowPack* pk,
                                         int slot_order, hipStream_t st) {
    return tri_attn_rowfused_run(ap, z, zb, zs, zl, pk, slot_order, st, nullptr);
}

extern "C" int abx_tri_attn_plan(const AbxTriAttn* ap, int rowfused, char* name, int cap) {
    ABX_REQUIRE(ap && name && cap > 0, "abx_tri_attn_plan: null descriptor or no room for the name");
    AbxPlan plan = {};
    // row-fused: the z rows lie where the descriptor's q rows would (strides sb / ss / sl); z and the row pack are stand-ins that pass the operand
    // checks - an address is looked at, never followed
    alignas(16) static const char stand_in[16] = {};
    const AbxTriRowPack pk = {reinterpret_cast<const unsigned short*>(stand_in), reinterpret_cast<const float*>(stand_in),
                              reinterpret_cast<const float*>(stand_in), 0, 4};
    if (int rc = rowfused ? tri_attn_rowfused_run(ap, reinterpret_cast<const float*>(stand_in), ap->sb, ap->ss, ap->sl, &pk, -1, nullptr, &plan)
                          : tri_attn_run(ap, nullptr, &plan))
        return rc;
    snprintf(name, (size_t)cap, "%s", plan.name);
    return ABX_OK;
}
