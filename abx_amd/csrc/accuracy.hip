// Accuracy of designs against the crystal structure (include/abx_hip.h, AbxAccuracyArgs): all-atom / backbone / C-alpha lDDT - the
// quantity pLDDT predicts (abx/model/utils.py:102-155) -, the TM block of TMscoreHead (abx/model/head.py:116-141, abx/utils.py:562-578,
// 525-560, 703-763) and the recovery of the native antibody-antigen residue contacts.  One row of ABX_ACC_COLS doubles per structure.
//
// Two kernels, no floating-point atomics, every float sum in a fixed order (a structure's row does not depend on its batch mates):
//   acc_pair_kernel  grid (residue tile, structure), the O((14 L)^2) part, tiled like metrics.hip::clash_count_kernel: a block owns 16
//                    residues (224 atoms, one thread each) and streams ALL column tiles of the wild type and of the design through LDS
//                    (ordered pairs: the counts are per row residue).  Both squared distances in float64 without fused multiply-add;
//                    the two square roots only for an included pair.  15 integer counters per thread (3 classes x (pairs, preserved
//                    at 0.5 / 1 / 2 / 4)), reduced to the residue with integer LDS adds; residue-contact bits of a tile pair by
//                    integer LDS or, counted per row residue after every antigen tile.  Integer adds commute: the counts are exact.
//   acc_row_kernel   one block per structure: the pooled integer sums (exact in float64), the pLDDT calibration, the C-alpha
//                    superposition (Horn's quaternion, cyclic Jacobi in LDS, as metrics.hip), the TM block, the row.
#include "common.h"
#include "abx_hip.h"
#include "reduce_dev.h"
#include "structure_dev.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int RT = 16;                 // residues per tile
constexpr int AT = RT * 14;            // atoms per tile (224)
constexpr int WS = 20;                 // ints per residue in the workspace: counts [3][5], n_native, n_kept, n_new, scored atoms, pad
constexpr int F_SCORED = 1, F_WILD = 2, F_DESIGN = 4;

// One design of the batch (structure_dev.h) and the wild type: the ground truth in every row
struct Structure : StructureView<AbxAccuracyArgs> {
    using StructureView<AbxAccuracyArgs>::StructureView;
    __device__ __forceinline__ int wild_aatype(int res) const { return clamp_aa(gseq[res]); }
    __device__ __forceinline__ const float* wild_xyz(int res, int slot) const { return gt + ((long long)res * 14 + slot) * 3; }
    __device__ __forceinline__ bool wild_exists(int res, int slot) const { return kept(res) && gexists[(long long)res * 14 + slot] != 0; }
};

__global__ __launch_bounds__(256) void acc_pair_kernel(const AbxAccuracyArgs a, int* __restrict__ ws) {
    __shared__ float4 wt[AT];          // wild type: x, y, z, flags (residue index << 8 | slot << 4 | F_*) as bits
    __shared__ float4 dt[AT];          // design: x, y, z
    __shared__ int rcnt[RT][WS];       // per row residue of this block
    __shared__ int cbits[RT * RT];     // contact bits of (row residue, column residue) of the current tile pair
    const int b = blockIdx.y, it = blockIdx.x, tid = threadIdx.x, L = a.L, Lab = a.Lab;
    const Structure s(a, b);
    auto load_atom = [&](int res, int slot, float4& w, float4& d) {
        w = make_float4(0.f, 0.f, 0.f, __int_as_float(0));
        d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (res < L) {
            const int aa = s.aatype(res);
            const bool we = s.wild_exists(res, slot), de = s.exists(res, slot, aa);
            const bool sc = we && de && (aa == s.wild_aatype(res) || slot <= 4);
            const float* xw = s.wild_xyz(res, slot);
            const float* xd = s.xyz(res, slot);
            const int f = (res << 8) | (slot << 4) | (sc ? F_SCORED : 0) | (we ? F_WILD : 0) | (de ? F_DESIGN : 0);
            w = make_float4(xw[0], xw[1], xw[2], __int_as_float(f));
            d = make_float4(xd[0], xd[1], xd[2], 0.f);
        }
    };
    for (int k = tid; k < RT * WS; k += 256) (&rcnt[0][0])[k] = 0;
    const int mloc = tid / 14, mslot = tid - mloc * 14, mres = it * RT + mloc;
    float4 mw = make_float4(0.f, 0.f, 0.f, 0.f), md = mw;
    int mf = 0;
    if (tid < AT) {
        load_atom(mres, mslot, mw, md);
        mf = __float_as_int(mw.w);
    }
    const double wx = (double)mw.x, wy = (double)mw.y, wz = (double)mw.z, px = (double)md.x, py = (double)md.y, pz = (double)md.z;
    const double r2 = a.lddt_radius * a.lddt_radius, c2 = a.contact * a.contact;
    const bool mside = mres < Lab;
    int c[3][5];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int k = 0; k < 5; ++k) c[q][k] = 0;
    const int nt = (L + RT - 1) / RT;
    for (int jt = 0; jt < nt; ++jt) {
        // antibody rows in this block and antigen rows in the column tile: the only tile pairs with residue contacts
        const bool cross = it * RT < Lab && jt * RT + RT - 1 >= Lab;
        __syncthreads();
        if (jt == it) {
            if (tid < AT) { wt[tid] = mw; dt[tid] = md; }
        } else if (tid < AT) {
            load_atom(jt * RT + tid / 14, tid % 14, wt[tid], dt[tid]);
        }
        if (cross) cbits[tid] = 0;
        __syncthreads();
        if (tid < AT && (mf & (F_WILD | F_DESIGN))) {
            for (int k = 0; k < AT; ++k) {
                const float4 ow = wt[k];
                const int of = __float_as_int(ow.w);
                const int both = mf & of;
                if (!(both & (F_WILD | F_DESIGN)) || (of >> 8) == mres) continue;
                const float4 od = dt[k];
                double dx = wx - (double)ow.x, dy = wy - (double)ow.y, dz = wz - (double)ow.z;
                const double d2w = (dx * dx + dy * dy) + dz * dz;
                dx = px - (double)od.x; dy = py - (double)od.y; dz = pz - (double)od.z;
                const double d2d = (dx * dx + dy * dy) + dz * dz;
                if ((both & F_SCORED) && d2w < r2) {
                    const double diff = fabs(sqrt(d2w) - sqrt(d2d));
                    const int oslot = (of >> 4) & 15;
                    const int p0 = diff < 0.5 ? 1 : 0, p1 = diff < 1.0 ? 1 : 0, p2 = diff < 2.0 ? 1 : 0, p3 = diff < 4.0 ? 1 : 0;
                    const int bb = (mslot <= 4 && oslot <= 4) ? 1 : 0, ca = (mslot == 1 && oslot == 1) ? 1 : 0;
                    c[0][0] += 1; c[0][1] += p0; c[0][2] += p1; c[0][3] += p2; c[0][4] += p3;
                    c[1][0] += bb; c[1][1] += bb & p0; c[1][2] += bb & p1; c[1][3] += bb & p2; c[1][4] += bb & p3;
                    c[2][0] += ca; c[2][1] += ca & p0; c[2][2] += ca & p1; c[2][3] += ca & p2; c[2][4] += ca & p3;
                }
                if (cross && mside && (of >> 8) >= Lab) {
                    const int bits = (((both & F_WILD) && d2w < c2) ? 1 : 0) | (((both & F_DESIGN) && d2d < c2) ? 2 : 0);
                    if (bits) atomicOr(&cbits[mloc * RT + ((of >> 8) - jt * RT)], bits);
                }
            }
        }
        if (cross) {
            __syncthreads();
            const int r = tid >> 4, cc = tid & 15, rres = it * RT + r, cres = jt * RT + cc;
            if (rres < Lab && cres >= Lab && cres < L) {
                const int bits = cbits[tid];
                if (a.contacts) a.contacts[((long long)b * Lab + rres) * (L - Lab) + (cres - Lab)] = (unsigned char)bits;
                if (bits & 1) atomicAdd(&rcnt[r][15], 1);
                if (bits == 3) atomicAdd(&rcnt[r][16], 1);
                if (bits == 2) atomicAdd(&rcnt[r][17], 1);
            }
        }
    }
    if (tid < AT) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (c[q][k]) atomicAdd(&rcnt[mloc][q * 5 + k], c[q][k]);
        if (mf & F_SCORED) atomicAdd(&rcnt[mloc][18], 1);
    }
    __syncthreads();
    for (int k = tid; k < RT * WS; k += 256) {
        const int res = it * RT + k / WS;
        if (res < L) ws[((long long)b * L + res) * WS + (k % WS)] = (&rcnt[0][0])[k];
    }
}

// sum of the four preserved counts of a class
__device__ __forceinline__ int preserved(const int* w, int q) { return (w[q * 5 + 1] + w[q * 5 + 2]) + (w[q * 5 + 3] + w[q * 5 + 4]); }

constexpr int NS = 22;
__global__ __launch_bounds__(256) void acc_row_kernel(const AbxAccuracyArgs a, const int* __restrict__ ws) {
    __shared__ double red[4 * NS];
    __shared__ double Nm[4][4], Vm[4][4];
    __shared__ double Rs[9];
    const int b = blockIdx.x, tid = threadIdx.x, L = a.L, Lab = a.Lab;
    const Structure s(a, b);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const float* pl = a.plddt ? a.plddt + (long long)b * a.plddt_sb : nullptr;
    // ---- pooled integer sums (exact in float64: below 2^53) and the pLDDT calibration
    // 0-1 all: pairs, preserved; 2-3 antibody; 4-5 region; 6-7 bb region; 8-9 ca all; 10-11 ca region; 12 scored atoms;
    // 13-15 native, kept, new; 16-17 native, kept of region rows; 18-19 sum plddt, rows; 20-21 sum |plddt - 100 lDDT-ca|, rows
    double v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = 0.0;
    for (int i = tid; i < L; i += 256) {
        int w[WS];
        const int* src = ws + ((long long)b * L + i) * WS;
#pragma unroll
        for (int k = 0; k < WS; ++k) w[k] = src[k];
        const bool reg = a.region && a.region[i] && s.kept(i);
        const double n_all = (double)w[0], p_all = (double)preserved(w, 0), n_bb = (double)w[5], p_bb = (double)preserved(w, 1);
        const double n_ca = (double)w[10], p_ca = (double)preserved(w, 2);
        const double l_ca = w[10] > 0 ? p_ca / (4.0 * n_ca) : nan;
        if (a.rows) {
            double* dst = a.rows + ((long long)b * L + i) * 4;
            dst[0] = w[0] > 0 ? p_all / (4.0 * n_all) : nan;
            dst[1] = w[5] > 0 ? p_bb / (4.0 * n_bb) : nan;
            dst[2] = l_ca;
            dst[3] = n_all;
        }
        if (a.counts) {
            int* dst = a.counts + ((long long)b * L + i) * 15;
#pragma unroll
            for (int k = 0; k < 15; ++k) dst[k] = w[k];
        }
        v[0] += n_all; v[1] += p_all;
        if (i < Lab) { v[2] += n_all; v[3] += p_all; }
        v[8] += n_ca; v[9] += p_ca;
        v[12] += (double)w[18];
        v[13] += (double)w[15]; v[14] += (double)w[16]; v[15] += (double)w[17];
        if (reg) {
            v[4] += n_all; v[5] += p_all;
            v[6] += n_bb; v[7] += p_bb;
            v[10] += n_ca; v[11] += p_ca;
            v[16] += (double)w[15]; v[17] += (double)w[16];
            if (pl) {
                const double p = (double)pl[i];
                v[18] += p; v[19] += 1.0;
                if (w[10] > 0) { v[20] += fabs(p - 100.0 * l_ca); v[21] += 1.0; }
            }
        }
    }
    block_sum_d<NS>(v, red);
    auto ratio = [&](double num, double den) { return den > 0.0 ? num / den : nan; };
    if (tid == 0) {                                     // written here: the 22 sums are dead before the superposition starts
        double* out = a.out + (long long)b * a.out_stride;
        out[0] = ratio(v[1], 4.0 * v[0]);
        out[1] = ratio(v[3], 4.0 * v[2]);
        out[2] = ratio(v[5], 4.0 * v[4]);
        out[3] = ratio(v[7], 4.0 * v[6]);
        out[4] = ratio(v[9], 4.0 * v[8]);
        out[5] = ratio(v[11], 4.0 * v[10]);
        out[6] = ratio(v[18], v[19]);
        out[7] = ratio(v[20], v[21]);
        out[12] = v[13]; out[13] = v[14];
        out[14] = ratio(v[14], v[13]);
        out[15] = v[15];
        out[16] = v[16]; out[17] = v[17];
        out[18] = ratio(v[17], v[16]);
        out[19] = v[4];
        out[20] = v[12];
    }
    // ---- centroids of the C-alpha of the rows that have one in the wild type
    auto ca_ok = [&](int i) { return s.wild_exists(i, 1); };
    double c0[7] = {0, 0, 0, 0, 0, 0, 0};               // n, wild type xyz, design xyz
    for (int i = tid; i < L; i += 256) {
        if (!ca_ok(i)) continue;
        const float* g = s.wild_xyz(i, 1);
        const float* p = s.xyz(i, 1);
        c0[0] += 1.0;
        c0[1] += (double)g[0]; c0[2] += (double)g[1]; c0[3] += (double)g[2];
        c0[4] += (double)p[0]; c0[5] += (double)p[1]; c0[6] += (double)p[2];
    }
    block_sum_d<7>(c0, red);
    const double nca = c0[0];
    const double cg[3] = {c0[1] / nca, c0[2] / nca, c0[3] / nca};
    const double cp[3] = {c0[4] / nca, c0[5] / nca, c0[6] / nca};
    // ---- covariance S[j][k] = sum (g_j - cg_j)(p_k - cp_k): the wild type is moved onto the design (the distances are those of the
    // opposite direction)
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < L; i += 256) {
        if (!ca_ok(i)) continue;
        const float* g = s.wild_xyz(i, 1);
        const float* p = s.xyz(i, 1);
        const double gx = (double)g[0] - cg[0], gy = (double)g[1] - cg[1], gz = (double)g[2] - cg[2];
        const double qx = (double)p[0] - cp[0], qy = (double)p[1] - cp[1], qz = (double)p[2] - cp[2];
        S[0] += gx * qx; S[1] += gx * qy; S[2] += gx * qz;
        S[3] += gy * qx; S[4] += gy * qy; S[5] += gy * qz;
        S[6] += gz * qx; S[7] += gz * qy; S[8] += gz * qz;
    }
    block_sum_d<9>(S, red);
    if (tid == 0 && nca > 0.0) horn_rotation_lds(S, Nm, Vm, Rs);
    __syncthreads();
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = nca > 0.0 ? Rs[k] : 0.0;
    // ---- the TM block: sum 1 / (1 + (d / d0)^2), sum d^2, the C-alpha within 0.5, 1, 2, 4, 8
    const double d0 = 1.24 * cbrt((nca > 21.0 ? nca : 21.0) - 15.0) - 1.8;
    double t[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < L; i += 256) {
        if (!ca_ok(i)) continue;
        const float* g = s.wild_xyz(i, 1);
        const float* p = s.xyz(i, 1);
        const double gx = (double)g[0] - cg[0], gy = (double)g[1] - cg[1], gz = (double)g[2] - cg[2];
        const double ex = ((R[0] * gx + R[1] * gy) + R[2] * gz) - ((double)p[0] - cp[0]);
        const double ey = ((R[3] * gx + R[4] * gy) + R[5] * gz) - ((double)p[1] - cp[1]);
        const double ez = ((R[6] * gx + R[7] * gy) + R[8] * gz) - ((double)p[2] - cp[2]);
        const double d2 = (ex * ex + ey * ey) + ez * ez;
        const double d = sqrt(d2), q = d / d0;
        t[0] += 1.0 / (1.0 + q * q);
        t[1] += d2;
        t[2] += d <= 0.5 ? 1.0 : 0.0; t[3] += d <= 1.0 ? 1.0 : 0.0; t[4] += d <= 2.0 ? 1.0 : 0.0;
        t[5] += d <= 4.0 ? 1.0 : 0.0; t[6] += d <= 8.0 ? 1.0 : 0.0;
    }
    block_sum_d<7>(t, red);
    if (tid == 0) {
        double* out = a.out + (long long)b * a.out_stride;
        out[8] = ratio(t[0], nca);
        out[9] = ratio((t[3] + t[4]) + (t[5] + t[6]), 4.0 * nca);
        out[10] = ratio((t[2] + t[3]) + (t[4] + t[5]), 4.0 * nca);
        out[11] = nca > 0.0 ? sqrt(t[1] / nca) : nan;
    }
}

}  // namespace

extern "C" long long abx_accuracy_scores_workspace_bytes(int B, int L) {
    if (B <= 0 || L <= 0) return 0;
    return (long long)B * L * WS * sizeof(int);
}

extern "C" int abx_accuracy_scores(const AbxAccuracyArgs* ap, void* workspace, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_accuracy_scores: null");
    const AbxAccuracyArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_accuracy_scores", 1, true)) return rc;
    ABX_REQUIRE(a.out, "abx_accuracy_scores: null operand");
    ABX_REQUIRE(a.out_stride >= ABX_ACC_COLS, "abx_accuracy_scores: out_stride below ABX_ACC_COLS");
    ABX_REQUIRE(std::isfinite(a.lddt_radius) && a.lddt_radius > 0.0, "abx_accuracy_scores: lddt_radius must be > 0");
    ABX_REQUIRE(std::isfinite(a.contact) && a.contact > 0.0, "abx_accuracy_scores: contact must be > 0");
    ABX_REQUIRE(workspace != nullptr, "abx_accuracy_scores: null workspace");
    int* ws = reinterpret_cast<int*>(workspace);
    hipLaunchKernelGGL(acc_pair_kernel, dim3((a.L + RT - 1) / RT, a.B), dim3(256), 0, st, a, ws);
    int rc = abx_check_launch("abx_accuracy_scores(pairs)");
    if (rc) return rc;
    hipLaunchKernelGGL(acc_row_kernel, dim3(a.B), dim3(256), 0, st, a, ws);
    return abx_check_launch("abx_accuracy_scores");
}
