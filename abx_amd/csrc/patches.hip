// Surface patches of designs (include/abx_hip.h, AbxPatchArgs): the patches of surface hydrophobicity and of positive / negative charge
// around the CDRs of the free antibody (rows < Lab), its Fv charge symmetry parameter, and the charge pairing across the interface.  One
// row of ABX_PATCH_COLS doubles per structure, equal bit for bit to abx_amd.patches.patches_host: every distance in float64 without
// fused multiply-add, every term a fixed-point integer, every sum an int64.
//
// Worst case of the integers (header, "Bounds"): a patch term is at most 2^30 h_max^2, a cross term at most 2^30 (q_max / 10)^2; there
// are at most Lab^2 / 2 patch pairs and Lab (L - Lab) cross pairs.  With the shipped tables (h <= 2, |q10| <= 10) and L <= MAX_L = 2048
// every sum stays below 2^53, so the final division by 2^30 is exact.  The entry refuses L > MAX_L (the row tables of the last kernel
// are static LDS) and tables with 2^30 h_max^2 Lab^2 or 2^30 (q_max / 10)^2 Lab L >= 2^62.
//
// Three kernels, no global atomics:
//   1. patch_flags_kernel, one workgroup per structure, one thread per row of the complex: type, presence, exposure
//      (residue_rules.h), seed, region, heavy chain; the counted atoms compacted to the front of the row's 14 float4 (x, y, z | role
//      bits) in the workspace, their number in the row's info word.
//   2. patch_pair_kernel, the hot path, grid (tile of 256 j-rows, tile of TI = 16 antibody i-rows, structure): one lane per j-row with its
//      atoms in registers as float64 (slots beyond its count at +inf: their distances are +inf and never the minimum), the atoms of the
//      i-rows in LDS, every lane reads the same address - a broadcast.  D2[i][j] to the (Lab, L) float64 plane of the workspace, and per
//      (i-tile, j-row) one byte: some i of the tile has S2[i][j] <= salt2.  D2 and S2 are symmetric, so "row j is salt-bridged" is the OR
//      of row j's bytes over the i-tiles.
//   3. patch_reduce_kernel, one workgroup per structure: salt-bridged rows, vicinity, the fixed-point terms (a wave per i-row, a lane per
//      j-row; int64 sums through LDS), SFvCSP, the cross terms, the per-row shares; writes the row and the optional (L, 4) table.
#include "common.h"
#include "abx_hip.h"
#include "reduce_dev.h"
#include "residue_rules.h"
#include "structure_dev.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                // threads of every workgroup
constexpr int NW = NT / 64;
constexpr int TI = 16;                 // antibody rows of a pair tile
constexpr int MAX_L = 2048;            // rows of a structure: the row tables of patch_reduce_kernel (56 KB of LDS)
// bits of a row's info word: type in bits 0-4, the number of counted atoms in bits 16-19
constexpr int R_PRESENT = 1 << 5, R_EXPOSED = 1 << 6, R_SEED = 1 << 7, R_VICINITY = 1 << 8, R_SALT = 1 << 9, R_REGION = 1 << 10,
              R_HEAVY = 1 << 11, R_CDR = 1 << 12;
constexpr int ROLES = ABX_POLAR_CATION | ABX_POLAR_ANION;
// columns of the row
constexpr int C_SFV = 3, C_NCDR = 11, C_NEXP = 12, C_NVIC = 13, C_NPAIRS = 14, C_NSALT = 15, C_NCROSS = 16, C_NCROSS_REG = 17;

using Structure = StructureView<AbxPatchArgs>;

// One structure's block of the workspace: the rows' atoms, the D2 plane, the info words, the salt bytes of every i-tile
struct Block {
    float4* atoms; double* d2; int* info; unsigned char* salt;
};
__host__ __device__ constexpr int tiles_of(int Lab) { return (Lab + TI - 1) / TI; }
__host__ __device__ constexpr long long block_bytes(int L, int Lab) {
    return (224ll * L + 8ll * Lab * L + 4ll * L + (long long)tiles_of(Lab) * Lab + 15) / 16 * 16;
}
__device__ __forceinline__ Block block_of(void* ws, int b, int L, int Lab) {
    unsigned char* p = static_cast<unsigned char*>(ws) + (long long)b * block_bytes(L, Lab);
    Block k;
    k.atoms = reinterpret_cast<float4*>(p);
    k.d2 = reinterpret_cast<double*>(k.atoms + 14ll * L);
    k.info = reinterpret_cast<int*>(k.d2 + (long long)Lab * L);
    k.salt = reinterpret_cast<unsigned char*>(k.info + L);
    return k;
}

__global__ __launch_bounds__(NT) void patch_flags_kernel(const AbxPatchArgs a, void* ws) {
    const int b = blockIdx.x, L = a.L, Lab = a.Lab;
    const Structure s(a, b);
    const Block k = block_of(ws, b, L, Lab);
    const int* pts = a.points + (long long)b * L * 28;
    const int heavy = a.chain_id[0];
    for (int r = threadIdx.x; r < L; r += NT) {
        const int aa = s.aatype(r);
        float4* at = k.atoms + 14ll * r;
        int n = 0;
        for (int sl = 0; sl < 14; ++sl) {
            const bool counted = a.radius[aa * 14 + sl] > 0.f && s.exists(r, sl, aa);
            if (counted) {
                const float* x = s.xyz(r, sl);
                at[n++] = make_float4(x[0], x[1], x[2], __int_as_float(a.table[aa * 14 + sl] & ROLES));
            }
        }
        for (int e = n; e < 14; ++e) at[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        int f = aa | n << 16;
        if (n) {
            f |= R_PRESENT | (a.region && a.region[r] ? R_REGION : 0);
            if (r < Lab) {
                const bool cdr = is_cdr(a.cdr_def[r]);
                f |= (a.chain_id[r] == heavy ? R_HEAVY : 0) | (cdr ? R_CDR : 0);
                if (row_exposed(sidechain_rel_area(s, a.radius, pts, a.a, r, aa), a.ref[aa], a.exposed)) f |= R_EXPOSED | (cdr ? R_SEED : 0);
            }
        }
        k.info[r] = f;
    }
}

__global__ __launch_bounds__(NT) void patch_pair_kernel(const AbxPatchArgs a, void* ws) {
    __shared__ float4 ia[TI * 14];
    __shared__ int in[TI];
    const int b = blockIdx.z, tid = threadIdx.x, L = a.L, Lab = a.Lab;
    const Block k = block_of(ws, b, L, Lab);
    const int i0 = blockIdx.y * TI, j = blockIdx.x * NT + tid;
    const int rows = Lab - i0 < TI ? Lab - i0 : TI;         // >= 1: the grid has tiles_of(Lab) i-tiles
    for (int e = tid; e < rows * 14; e += NT) ia[e] = k.atoms[14ll * i0 + e];
    if (tid < rows) in[tid] = k.info[i0 + tid] >> 16 & 15;
    // the lane's own row: 14 atoms as float64, the slots beyond its count at +inf
    double xj[14], yj[14], zj[14];
    int catj = 0, anj = 0;
    const int nj = j < L ? k.info[j] >> 16 & 15 : 0;
#pragma unroll
    for (int e = 0; e < 14; ++e) {
        xj[e] = yj[e] = zj[e] = INFINITY;
        if (e < nj) {
            const float4 p = k.atoms[14ll * j + e];
            xj[e] = (double)p.x; yj[e] = (double)p.y; zj[e] = (double)p.z;
            const int role = __float_as_int(p.w);
            catj |= (role & ABX_POLAR_CATION) ? 1 << e : 0;
            anj |= (role & ABX_POLAR_ANION) ? 1 << e : 0;
        }
    }
    __syncthreads();
    if (blockIdx.x * NT + (tid & ~63) >= L) return;         // a whole wave beyond the last row; no barrier follows
    const double salt2 = a.salt2;
    bool salted = false;
    for (int r = 0; r < rows; ++r) {
        const int i = i0 + r, ni = in[r];
        double m = INFINITY, sm = INFINITY;
        for (int e = 0; e < ni; ++e) {
            const float4 p = ia[r * 14 + e];
            const double xi = (double)p.x, yi = (double)p.y, zi = (double)p.z;
            const int role = __builtin_amdgcn_readfirstlane(__float_as_int(p.w));
            if (role == 0) {                                // (uniform: the i-atom is the same for every lane)
#pragma unroll
                for (int c = 0; c < 14; ++c) {
                    const double dx = xj[c] - xi, dy = yj[c] - yi, dz = zj[c] - zi;
                    m = fmin(m, (dx * dx + dy * dy) + dz * dz);
                }
            } else {                                        // a charged atom: its partners are the lane's atoms of the other role
                const int partner = (role & ABX_POLAR_CATION ? anj : 0) | (role & ABX_POLAR_ANION ? catj : 0);
#pragma unroll
                for (int c = 0; c < 14; ++c) {
                    const double dx = xj[c] - xi, dy = yj[c] - yi, dz = zj[c] - zi;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    m = fmin(m, d2);
                    sm = fmin(sm, (partner >> c & 1) ? d2 : INFINITY);
                }
            }
        }
        if (j < L) k.d2[(long long)i * L + j] = j == i ? INFINITY : m;
        if (j != i && sm <= salt2) salted = true;
    }
    if (j < Lab) k.salt[(long long)blockIdx.y * Lab + j] = salted ? 1 : 0;
}

__global__ __launch_bounds__(NT) void patch_reduce_kernel(const AbxPatchArgs a, void* ws) {
    __shared__ int info[MAX_L];
    __shared__ unsigned long long psh[MAX_L], chg[MAX_L], crs[MAX_L];       // the rows' shares (two's complement)
    __shared__ unsigned long long tot[10];              // psh, ppc, pnc, their region sums, attract, repel, their region sums
    __shared__ int cnt[ABX_PATCH_COLS + 2];             // the count columns by their column; [0], [1]: the two charge sums of SFvCSP
    __shared__ double h[21];
    __shared__ int q10[21];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = a.L, Lab = a.Lab;
    const Block k = block_of(ws, b, L, Lab);
    for (int r = tid; r < L; r += NT) {
        info[r] = k.info[r];
        psh[r] = chg[r] = crs[r] = 0ull;
    }
    if (tid < 10) tot[tid] = 0ull;
    if (tid < ABX_PATCH_COLS + 2) cnt[tid] = 0;
    if (tid < 21) {
        h[tid] = a.h[tid];
        q10[tid] = a.q10[tid];
    }
    __syncthreads();
    // ---- salt-bridged rows; CDR length, exposed rows, the charge sums of the two chains
    const int nit = tiles_of(Lab);
    for (int r = tid; r < Lab; r += NT) {
        int f = info[r];
        if (!(f & R_PRESENT)) continue;
        bool salted = false;
        for (int t = 0; t < nit; ++t) salted = salted || k.salt[(long long)t * Lab + r] != 0;
        if (salted) info[r] = f | R_SALT;
        if (f & R_CDR) atomicAdd(&cnt[C_NCDR], 1);
        if (f & R_EXPOSED) {
            atomicAdd(&cnt[C_NEXP], 1);
            const int q = q10[f & 31];
            if (q) atomicAdd(&cnt[(f & R_HEAVY) ? 0 : 1], q);
        }
    }
    __syncthreads();
    // ---- vicinity: a wave per exposed row, a lane per seed
    const double vic2 = a.vicinity2, cut2 = a.cutoff2;
    for (int i = wv; i < Lab; i += NW) {
        const int f = info[i];
        if (!(f & R_EXPOSED)) continue;
        bool near = (f & R_SEED) != 0;
        if (!near) {
            for (int s = lane; s < Lab; s += 64)
                if ((info[s] & R_SEED) && k.d2[(long long)i * L + s] <= vic2) near = true;
            near = __any(near);
        }
        if (near && lane == 0) {
            atomicOr(&info[i], R_VICINITY);
            atomicAdd(&cnt[C_NVIC], 1);
            if (f & R_SALT) atomicAdd(&cnt[C_NSALT], 1);
        }
    }
    __syncthreads();
    // ---- patch terms: a wave per vicinity row i, a lane per vicinity row j > i
    long long t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int n_pairs = 0, n_cross = 0, n_cross_reg = 0;
    for (int i = wv; i < Lab; i += NW) {
        const int fi = info[i];
        if (!(fi & R_VICINITY)) continue;
        const int qi = q10[fi & 31];
        const double hi = h[(fi & R_SALT) ? a.gly : (fi & 31)], Qi = (double)qi / 10.0;
        for (int j = i + 1 + lane; j < Lab; j += 64) {
            const int fj = info[j];
            if (!(fj & R_VICINITY)) continue;
            const double d2 = k.d2[(long long)i * L + j];
            if (!(d2 <= cut2)) continue;
            const double r2 = d2 > 1.0 ? d2 : 1.0;
            const int qj = q10[fj & 31];
            const double hj = h[(fj & R_SALT) ? a.gly : (fj & 31)], Qj = (double)qj / 10.0;
            const bool reg = ((fi | fj) & R_REGION) != 0;
            const long long term = llrint(FIXED_ONE * ((hi * hj) / r2));
            const long long c = llrint(FIXED_ONE * (fabs(Qi * Qj) / r2));
            ++n_pairs;
            t[0] += term;
            t[3] += reg ? term : 0;
            lds_add(&psh[i], term);
            lds_add(&psh[j], term);
            const int sign = (qi > 0 && qj > 0) ? 1 : ((qi < 0 && qj < 0) ? 2 : 0);
            if (sign) {
                t[sign] += c;
                t[3 + sign] += reg ? c : 0;
                lds_add(&chg[i], c);
                lds_add(&chg[j], c);
            }
        }
    }
    // ---- across the interface: a wave per charged antibody row, a lane per antigen row
    for (int i = wv; i < Lab; i += NW) {
        const int fi = info[i], qi = q10[fi & 31];
        if (!(fi & R_PRESENT) || qi == 0) continue;
        const double Qi = (double)qi / 10.0;
        for (int j = Lab + lane; j < L; j += 64) {
            const int fj = info[j], qj = q10[fj & 31];
            if (!(fj & R_PRESENT) || qj == 0) continue;
            const double d2 = k.d2[(long long)i * L + j];
            if (!(d2 <= cut2)) continue;
            const double r2 = d2 > 1.0 ? d2 : 1.0;
            const double Qj = (double)qj / 10.0;
            const long long c = llrint(FIXED_ONE * (fabs(Qi * Qj) / r2));
            const int col = (qi > 0) != (qj > 0) ? 6 : 7;
            const long long share = col == 6 ? c : -c;
            t[col] += c;
            ++n_cross;
            if (fi & R_REGION) {
                t[col + 2] += c;
                ++n_cross_reg;
            }
            lds_add(&crs[i], share);
            lds_add(&crs[j], share);
        }
    }
    for (int c = 0; c < 10; ++c)
        if (t[c]) lds_add(&tot[c], t[c]);
    if (n_pairs) atomicAdd(&cnt[C_NPAIRS], n_pairs);
    if (n_cross) atomicAdd(&cnt[C_NCROSS], n_cross);
    if (n_cross_reg) atomicAdd(&cnt[C_NCROSS_REG], n_cross_reg);
    __syncthreads();
    if (tid < ABX_PATCH_COLS) {
        double v;
        if (tid < C_SFV) v = (double)(long long)tot[tid] / FIXED_ONE;
        else if (tid == C_SFV) v = (double)((long long)cnt[0] * (long long)cnt[1]) / 100.0;
        else if (tid < C_NCDR) v = (double)(long long)tot[tid - 1] / FIXED_ONE;
        else v = (double)cnt[tid];
        a.out[(long long)b * a.out_stride + tid] = v;
    }
    if (a.rows)
        for (int r = tid; r < L; r += NT) {
            const int f = info[r];
            double* o = a.rows + ((long long)b * L + r) * 4;
            o[0] = (double)(long long)psh[r] / FIXED_ONE;
            o[1] = (double)(long long)chg[r] / FIXED_ONE;
            o[2] = (double)(long long)crs[r] / FIXED_ONE;
            o[3] = (double)(((f & R_PRESENT) ? 1 : 0) | ((f & R_EXPOSED) ? 2 : 0) | ((f & R_SEED) ? 4 : 0) | ((f & R_VICINITY) ? 8 : 0) |
                            ((f & R_SALT) ? 16 : 0) | ((f & R_REGION) ? 32 : 0));
        }
}

}  // namespace

extern "C" long long abx_patch_scores_workspace_bytes(int B, int L, int Lab) {
    return B > 0 && L > 0 && Lab > 0 && Lab <= L ? (long long)B * block_bytes(L, Lab) : 0;
}

extern "C" int abx_patch_scores(const AbxPatchArgs* ap, void* workspace, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_patch_scores: null");
    const AbxPatchArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_patch_scores", 1)) return rc;
    ABX_REQUIRE(a.points && a.chain_id && a.cdr_def && a.h && a.q10 && a.table && a.a && a.ref && a.out && workspace,
                "abx_patch_scores: null operand");
    ABX_REQUIRE(a.out_stride >= ABX_PATCH_COLS, "abx_patch_scores: out_stride below ABX_PATCH_COLS");
    ABX_REQUIRE(std::isfinite(a.cutoff2) && a.cutoff2 > 0.0 && std::isfinite(a.vicinity2) && a.vicinity2 > 0.0 && std::isfinite(a.salt2) &&
                    a.salt2 > 0.0, "abx_patch_scores: cutoff2, vicinity2 and salt2 must be > 0");
    ABX_REQUIRE(std::isfinite(a.exposed) && a.exposed >= 0.0 && a.exposed <= 1.0, "abx_patch_scores: exposed must be in [0, 1]");
    ABX_REQUIRE(a.gly >= 0 && a.gly <= 20, "abx_patch_scores: gly must be a residue type (0..20)");
    ABX_REQUIRE(a.L <= MAX_L, "abx_patch_scores: the row tables do not fit the LDS (Lab <= L <= 2048)");
    const double q = (double)a.q_max / 10.0;
    ABX_REQUIRE(std::isfinite(a.h_max) && a.h_max >= 0.0 && a.q_max >= 0 &&
                    FIXED_ONE * a.h_max * a.h_max * (double)a.Lab * (double)a.Lab < 4.6e18 && FIXED_ONE * q * q * (double)a.Lab * (double)a.L < 4.6e18,
                "abx_patch_scores: the sums could leave int64 (2^30 h_max^2 Lab^2 or 2^30 (q_max / 10)^2 Lab L >= 2^62)");
    // the vicinity pairs of a salt-bridged row take h[gly], which h_max covers
    hipLaunchKernelGGL(patch_flags_kernel, dim3(a.B), dim3(NT), 0, st, a, workspace);
    if (int rc = abx_check_launch("abx_patch_scores")) return rc;
    hipLaunchKernelGGL(patch_pair_kernel, dim3((a.L + NT - 1) / NT, tiles_of(a.Lab), a.B), dim3(NT), 0, st, a, workspace);
    if (int rc = abx_check_launch("abx_patch_scores")) return rc;
    hipLaunchKernelGGL(patch_reduce_kernel, dim3(a.B), dim3(NT), 0, st, a, workspace);
    return abx_check_launch("abx_patch_scores");
}
