// Distogram head (include/abx_hip.h, AbxDistogramArgs): the 192 -> 64 projection of the pair representation, symmetrised, and what
// a design's confidence table needs from its softmax - without the (B, L, L, 64) logits ever reaching memory
// (abx/model/head.py:26-44, the contact definition of head.py:99-102).
//
// The projection is linear, so logits[i][j] = (0.5 (z[i][j] + z[j][i])) W + b: the OPERAND is symmetrised (0.5f * (a + b) commutes, so
// (i, j) and (j, i) multiply the same bits) and one product per pair remains.
//
//   disto_row_kernel<MODE>  grid (L, B), 4 waves: the workgroup owns row i of design b and walks the j tiles (64 pairs) in ascending
//                           order.  W (48 KB, packed per MFMA fragment by the caller) stays in LDS; a tile stages 0.5f * (z[b][i][j] +
//                           z[b][j][i]) as [64][196] floats (row stride 196: the 16 rows x 4 k of an A fragment fall into 64
//                           different banks).  Wave w multiplies the pairs 16 w .. 16 w + 15 by W with v_mfma_f32_16x16x4_f32 (exact
//                           fp32, k ascending): 4 accumulators = the 64 bins of 16 pairs, lane (g, c) holding the bins c + 16 t of the
//                           pairs 4 g + r.  MODE 1 stores them (abx_distogram_logits).  MODE 0 reduces them in registers: maximum and
//                           sums over a pair's bins by an xor butterfly over its 16 lanes, expf in fp32 of an exact float64 difference,
//                           every sum after it in float64.  The per-row sums of a lane run over the tiles in order, then over the
//                           lanes in order (LDS, fixed order): no atomics.
//   disto_reduce_kernel     one wave per design: `rows` from the per-row sums, then the table by a walk over the rows in ascending i.
#include "common.h"
#include "abx_hip.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int C = ABX_DISTO_CHANNELS;       // 192
constexpr int NB = ABX_DISTO_BINS;          // 64
constexpr int TJ = 64;                      // pairs of a tile
constexpr int LDZ = 196;                    // floats per staged pair
constexpr int NS = ABX_DISTO_ROWSUMS;       // per-row sums
constexpr int W_FLOATS = C * NB;
constexpr int Z_FLOATS = TJ * LDZ;
constexpr int LDS_BYTES = (W_FLOATS + Z_FLOATS + TJ * 4 + 3 * NB) * 4 + TJ * 4 + 16 * NS * 8;

// the per-row sums (workspace, (B, L, NS) float64)
enum { S_NLL = 0, N_ALL, S_NLL_AG, N_AG, S_DERR, N_DERR, S_ENT, S_PC_AG, N_CONTACT_AG, S_PC_CONTACT_AG };

template <typename T>
__device__ __forceinline__ T group16_sum(T v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int MODE>
__global__ __launch_bounds__(256) void disto_row_kernel(const AbxDistogramArgs a, float* __restrict__ logits_out) {
    extern __shared__ __align__(16) unsigned char lds[];
    float* Ws = reinterpret_cast<float*>(lds);                  // [48][4][64] fragments of W
    float* Zs = Ws + W_FLOATS;                                  // [64][LDZ] symmetrised operand of the tile
    float* Pj = Zs + Z_FLOATS;                                  // [64][4] pseudo-beta of j
    float* Bk = Pj + TJ * 4;                                    // [64] breaks (entry 63: +inf), [64] squared breaks, [64] bias
    int* Fj = reinterpret_cast<int*>(Bk + 3 * NB);              // [64] valid << 8 | class bits of j
    double* Red = reinterpret_cast<double*>(Fj + TJ);           // [16][NS]

    const int L = a.L, i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
    const float* zb = a.z + (long long)b * L * L * C;

    for (int k = tid; k < W_FLOATS / 4; k += 256) reinterpret_cast<float4*>(Ws)[k] = reinterpret_cast<const float4*>(a.W)[k];
    if (tid < NB) {
        Bk[2 * NB + tid] = a.bias[tid];
        if (MODE == 0) {
            Bk[tid] = tid < NB - 1 ? a.breaks[tid] : INFINITY;
            Bk[NB + tid] = tid < NB - 1 ? a.sq_breaks[tid] : INFINITY;
        }
    }
    __syncthreads();

    float bias_l[4], sqb_l[4];
    double cen_l[4];
    bool contact_l[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int k = t * 16 + c;
        bias_l[t] = Bk[2 * NB + k];
        sqb_l[t] = 0.f; cen_l[t] = 0.0; contact_l[t] = false;
        if (MODE == 0) {
            sqb_l[t] = Bk[NB + k];
            // bin k holds breaks[k-1] < d <= breaks[k]; its centre is the midpoint, the open end bins extend by half a step
            const double lo = (double)Bk[max(k - 1, 0)], hi = (double)Bk[min(k, NB - 2)];
            cen_l[t] = k == 0 ? (double)Bk[0] - 0.5 * ((double)Bk[1] - (double)Bk[0])
                     : k == NB - 1 ? (double)Bk[NB - 2] + 0.5 * ((double)Bk[NB - 2] - (double)Bk[NB - 3])
                                   : 0.5 * (lo + hi);
            // sum(pred[..., :t+1]) with t = #{breaks <= cutoff} (head.py:100-102): bin k enters iff k = 0 or breaks[k-1] <= cutoff
            contact_l[t] = k == 0 || Bk[k - 1] <= a.cutoff;
        }
    }

    bool vi = false;
    float xi = 0.f, yi = 0.f, zi = 0.f, cut2 = 0.f;
    if (MODE == 0) {
        vi = a.valid[(long long)b * L + i] != 0;
        const float* p = a.pb + ((long long)b * L + i) * 3;
        xi = p[0]; yi = p[1]; zi = p[2];
        cut2 = __fmul_rn(a.cutoff, a.cutoff);
    }
    double acc_s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc_s[k] = 0.0;
    const bool planes = MODE == 0 && (a.p_contact != nullptr || a.exp_dist != nullptr);
    const bool work = MODE == 1 || vi || planes;                // (uniform over the workgroup)

    for (int j0 = 0; work && j0 < L; j0 += TJ) {
        __syncthreads();                                        // the previous tile has been consumed
        // stage: 64 pairs x 48 float4, thread -> (pair, chunk) with the chunk fastest (768 contiguous bytes per pair and slice)
        for (int e = tid; e < TJ * (C / 4); e += 256) {
            const int p = e / (C / 4), q = e - p * (C / 4), j = j0 + p;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < L) {
                const float4 r = *reinterpret_cast<const float4*>(zb + ((long long)i * L + j) * C + q * 4);
                const float4 t = *reinterpret_cast<const float4*>(zb + ((long long)j * L + i) * C + q * 4);
                s = make_float4(0.5f * (r.x + t.x), 0.5f * (r.y + t.y), 0.5f * (r.z + t.z), 0.5f * (r.w + t.w));
            }
            *reinterpret_cast<float4*>(Zs + p * LDZ + q * 4) = s;
        }
        if (MODE == 0 && tid < TJ) {
            const int j = j0 + tid;
            int f = 0;
            float x = 0.f, y = 0.f, z = 0.f;
            if (j < L) {
                f = ((a.valid[(long long)b * L + j] != 0 && j != i) ? 256 : 0) | (int)a.classes[j];
                const float* p = a.pb + ((long long)b * L + j) * 3;
                x = p[0]; y = p[1]; z = p[2];
            }
            Fj[tid] = f;
            Pj[tid * 4] = x; Pj[tid * 4 + 1] = y; Pj[tid * 4 + 2] = z;
        }
        __syncthreads();

        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* za = Zs + (w * 16 + c) * LDZ + g;          // A[row = lane & 15][k = lane >> 4]
        const float* wb = Ws + lane;                            // B[k = lane >> 4][col = lane & 15] of fragment (kk, t)
#pragma unroll 4
        for (int kk = 0; kk < C / 4; ++kk) {
            const float av = za[kk * 4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wb[(kk * 4 + t) * 64], acc[t], 0, 0, 0);
        }

        // C/D of 16x16x4: element r of lane (g, c) is row 4 g + r, column c
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = w * 16 + g * 4 + r, j = j0 + p;
            float lg[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) lg[t] = acc[t][r] + bias_l[t];
            if (MODE == 1) {
                if (j < L) {
                    float* dst = logits_out + (((long long)b * L + i) * L + j) * NB + c;
#pragma unroll
                    for (int t = 0; t < 4; ++t) dst[t * 16] = lg[t];
                }
                continue;
            }
            float m = fmaxf(fmaxf(lg[0], lg[1]), fmaxf(lg[2], lg[3]));
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            // the realised bin: sum_k (d2 > breaks_k^2) in the operation order of abx_prev_pos
            const float dx = __fsub_rn(xi, Pj[p * 4]), dy = __fsub_rn(yi, Pj[p * 4 + 1]), dz = __fsub_rn(zi, Pj[p * 4 + 2]);
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            int part = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) part += d2 > sqb_l[t] ? 1 : 0;          // (entry 63 is +inf)
            const int bin = group16_sum(part);
            double s = 0.0, sc = 0.0, sd = 0.0, sl = 0.0, lr = 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double x = (double)lg[t] - (double)m;     // exact
                const double e = (double)expf((float)x);
                s += e;
                sc += contact_l[t] ? e : 0.0;
                sd += e * cen_l[t];
                sl += e * x;
                lr += (t * 16 + c == bin) ? x : 0.0;
            }
            s = group16_sum(s); sc = group16_sum(sc); sd = group16_sum(sd); sl = group16_sum(sl); lr = group16_sum(lr);
            const double pc = sc / s, ed = sd / s, lns = log(s);
            const double ent = lns - sl / s, nll = lns - lr;
            if (planes && c == 0 && j < L) {
                const long long o = ((long long)b * L + i) * L + j;
                if (a.p_contact) a.p_contact[o] = (float)pc;
                if (a.exp_dist) a.exp_dist[o] = (float)ed;
            }
            const int fj = Fj[p];
            if (vi && (fj & 256)) {
                acc_s[S_NLL] += nll; acc_s[N_ALL] += 1.0; acc_s[S_ENT] += ent;
                if (fj & ABX_DISTO_ANTIGEN) {
                    acc_s[S_NLL_AG] += nll; acc_s[N_AG] += 1.0; acc_s[S_PC_AG] += pc;
                    if (d2 < cut2) { acc_s[N_CONTACT_AG] += 1.0; acc_s[S_PC_CONTACT_AG] += pc; }
                }
                if (bin < NB - 1) { acc_s[S_DERR] += fabs(ed - sqrt((double)d2)); acc_s[N_DERR] += 1.0; }
            }
        }
    }
    if (MODE == 1) return;

    // lanes of a group hold equal sums; group (w, g) publishes, then a fixed-order sum over the 16 groups
    __syncthreads();
    if (c == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) Red[(w * 4 + g) * NS + k] = acc_s[k];
    }
    __syncthreads();
    if (tid < NS) {
        double v = 0.0;
        for (int q = 0; q < 16; ++q) v += Red[q * NS + tid];
        a.rowsums[((long long)b * L + i) * NS + tid] = v;
    }
}

// which per-row sum and which rows (class bits; 0: every row) a total takes
__constant__ int TOTAL_SRC[14] = {S_NLL, N_ALL, S_NLL_AG, N_AG, S_NLL, N_ALL, S_NLL_AG, N_AG, S_DERR, N_DERR, S_ENT, S_PC_AG, N_CONTACT_AG, S_PC_CONTACT_AG};
__constant__ int TOTAL_CLS[14] = {0, 0, ABX_DISTO_ANTIBODY, ABX_DISTO_ANTIBODY, ABX_DISTO_DESIGNED, ABX_DISTO_DESIGNED, ABX_DISTO_DESIGNED,
                                  ABX_DISTO_DESIGNED, ABX_DISTO_DESIGNED, ABX_DISTO_DESIGNED, ABX_DISTO_DESIGNED, ABX_DISTO_DESIGNED,
                                  ABX_DISTO_DESIGNED, ABX_DISTO_DESIGNED};

__global__ __launch_bounds__(64) void disto_reduce_kernel(const AbxDistogramArgs a) {
    __shared__ double tot[14];
    const int b = blockIdx.x, tid = threadIdx.x, L = a.L;
    const double* rs = a.rowsums + (long long)b * L * NS;
    if (a.rows) {
        for (int i = tid; i < L; i += 64) {
            const double* r = rs + (long long)i * NS;
            double* o = a.rows + ((long long)b * L + i) * 4;
            const double n = r[N_ALL];
            o[0] = n > 0.0 ? r[S_NLL] / n : 0.0;
            o[1] = r[S_PC_AG];
            o[2] = r[N_CONTACT_AG];
            o[3] = n > 0.0 ? r[S_ENT] / n : 0.0;
        }
    }
    if (tid < 14) {
        const int src = TOTAL_SRC[tid], cls = TOTAL_CLS[tid];
        double v = 0.0;
        for (int i = 0; i < L; ++i)                                 // ascending i
            if (cls == 0 || (a.classes[i] & cls)) v += rs[(long long)i * NS + src];
        tot[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double* o = a.table + (long long)b * a.table_stride;
        const auto mean = [](double s, double n) { return n > 0.0 ? s / n : 0.0; };
        o[0] = mean(tot[0], tot[1]);        // nll_all
        o[1] = mean(tot[2], tot[3]);        // nll_antibody_antigen
        o[2] = mean(tot[4], tot[5]);        // nll_region
        o[3] = mean(tot[6], tot[7]);        // nll_region_antigen
        o[4] = mean(tot[8], tot[9]);        // dist_err_region
        o[5] = mean(tot[10], tot[5]);       // entropy_region
        o[6] = tot[11];                     // exp_contacts_region_antigen
        o[7] = tot[12];                     // n_contacts_region_antigen
        o[8] = mean(tot[13], tot[12]);      // p_on_contacts_region_antigen
        o[9] = tot[5];                      // n_pairs_region
    }
}

int check_common(const AbxDistogramArgs& a, const char* what) {
    (void)what;
    ABX_REQUIRE(a.B > 0 && a.L > 0 && a.B <= 65535, "abx_distogram: bad sizes");
    ABX_REQUIRE((long long)a.L * a.L * ABX_DISTO_BINS < (1ll << 40), "abx_distogram: L too large");
    ABX_REQUIRE(a.z && a.W && a.bias, "abx_distogram: null operand");
    ABX_REQUIRE((reinterpret_cast<uintptr_t>(a.z) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.W) & 15) == 0,
                "abx_distogram: z and W must be 16-byte aligned");
    return ABX_OK;
}

}  // namespace

extern "C" int abx_distogram_scores(const AbxDistogramArgs* ap, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_distogram_scores: null");
    const AbxDistogramArgs a = *ap;
    int rc = check_common(a, "abx_distogram_scores");
    if (rc) return rc;
    ABX_REQUIRE(a.breaks && a.sq_breaks && a.pb && a.classes && a.valid, "abx_distogram_scores: null operand");
    ABX_REQUIRE(a.num_breaks == ABX_DISTO_BINS - 1, "abx_distogram_scores: num_breaks must be ABX_DISTO_BINS - 1");
    ABX_REQUIRE(std::isfinite(a.cutoff) && a.cutoff > 0.f, "abx_distogram_scores: cutoff must be > 0");
    ABX_REQUIRE(a.table && a.rowsums, "abx_distogram_scores: null table / rowsums");
    ABX_REQUIRE(a.table_stride >= ABX_DISTO_COLS, "abx_distogram_scores: table_stride below ABX_DISTO_COLS");
    rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(disto_row_kernel<0>), LDS_BYTES, "abx_distogram_scores");
    if (rc) return rc;
    hipLaunchKernelGGL(disto_row_kernel<0>, dim3(a.L, a.B), dim3(256), LDS_BYTES, st, a, nullptr);
    rc = abx_check_launch("abx_distogram_scores(rows)");
    if (rc) return rc;
    hipLaunchKernelGGL(disto_reduce_kernel, dim3(a.B), dim3(64), 0, st, a);
    return abx_check_launch("abx_distogram_scores");
}

extern "C" int abx_distogram_logits(const AbxDistogramArgs* ap, float* logits, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_distogram_logits: null");
    const AbxDistogramArgs a = *ap;
    int rc = check_common(a, "abx_distogram_logits");
    if (rc) return rc;
    ABX_REQUIRE(logits != nullptr, "abx_distogram_logits: null output");
    rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(disto_row_kernel<1>), LDS_BYTES, "abx_distogram_logits");
    if (rc) return rc;
    hipLaunchKernelGGL(disto_row_kernel<1>, dim3(a.L, a.B), dim3(256), LDS_BYTES, st, a, logits);
    return abx_check_launch("abx_distogram_logits");
}
