// Developability of designs (include/abx_hip.h, AbxDevelopabilityArgs): spatial aggregation propensity, chain charges and sequence
// liabilities of the free antibody (rows < Lab).  One row of ABX_DEV_COLS doubles per structure, equal bit for bit to
// abx_amd.developability.developability_host: every distance test in float64 without fused multiply-add, every sum an int64.
//
// Worst case of the integers (header, "Bounds"): |w_j| <= P q_max, which the shipped tables keep below 0.5 * 2^30 at P = 1024 as at the
// default of 128 (q shrinks as P grows); at most 10 weighted and 14 counted atoms per row, so |SAP_i| < 5 * 2^30 Lab and a structure's
// sum < 70 * 2^30 Lab^2: below 2^53 (the final division by 2^30 is exact) up to Lab = 346, below 2^63 for every accepted Lab.  The
// entry refuses 140 P q_max Lab^2 >= 2^63 and Lab > MAX_ROWS = 2048 (the row tables of the last kernel are static LDS).
//
// Three kernels, no global atomics:
//   1. dev_weigh_kernel, one workgroup per structure: w_j = acc_alone_j q[type][slot] of every counted atom; all counted atoms are
//      compacted (ballot prefix sums, slot order) into the i-list (x, y, z, row * 14 + slot), those with w != 0 into the j-list
//      (x, y, z | w); the two counts close the structure's workspace block.
//   2. dev_pair_kernel, grid (tile of 256 i-atoms, structure): one thread per atom i, the j-list through LDS in chunks of j_chunk atoms
//      ((3 x 4 + 8) bytes an atom: 40 KB at the default of 2048, four workgroups of a CU's 160 KB), every lane reads the same j - a
//      broadcast.  SAP_i to the workspace.  An empty j-list is never read.
//   3. dev_reduce_kernel, one workgroup per structure: row sums and atom counts by integer LDS atomics, the positive parts, the maximum
//      of the row means, charges, exposure, motifs over linked rows, free cysteines; writes the row and the optional (L, 4) table.
#include "common.h"
#include "abx_hip.h"
#include "peptide_dev.h"
#include "reduce_dev.h"
#include "residue_rules.h"
#include "structure_dev.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                // threads of every workgroup
constexpr int NW = NT / 64;
constexpr int J_CHUNK = 2048;          // default and largest chunk of the j-list in LDS
constexpr int MAX_ROWS = 2048;         // antibody rows of a structure
constexpr double CYS_SS2 = 6.25;
// bits of a row's info word: type in bits 0-4
constexpr int R_PRESENT = 1 << 5, R_EXPOSED = 1 << 6, R_LINK = 1 << 7, R_REGION = 1 << 8, R_CDR = 1 << 9, R_SG = 1 << 10;

using Structure = StructureView<AbxDevelopabilityArgs>;

// One structure's block of the workspace: i-list, j-list coordinates, j-list weights, SAP_i, the two counts
struct Block {
    float4* ilist; float4* jxyz; long long* jw; long long* sap; int* counts;
};
__host__ __device__ constexpr long long block_bytes(int Lab) { return 48ll * 14 * Lab + 16; }
__device__ __forceinline__ Block block_of(void* ws, int b, int Lab) {
    unsigned char* p = static_cast<unsigned char*>(ws) + (long long)b * block_bytes(Lab);
    const long long n = 14ll * Lab;
    Block k;
    k.ilist = reinterpret_cast<float4*>(p);
    k.jxyz = k.ilist + n;
    k.jw = reinterpret_cast<long long*>(k.jxyz + n);
    k.sap = k.jw + n;
    k.counts = reinterpret_cast<int*>(k.sap + n);
    return k;
}

__global__ __launch_bounds__(NT) void dev_weigh_kernel(const AbxDevelopabilityArgs a, void* ws) {
    __shared__ int wcnt[NW * 2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N14 = a.Lab * 14;
    const Structure s(a, b);
    const Block k = block_of(ws, b, a.Lab);
    const int* pts = a.points + (long long)b * a.L * 28;
    int n[2] = {0, 0};                                  // the i-list and the j-list so far
    for (int base = 0; base < N14; base += NT) {
        const int at = base + tid;
        bool counted = false;
        long long w = 0;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (at < N14) {
            const int row = at / 14, sl = at - row * 14, aa = s.aatype(row);
            counted = a.radius[aa * 14 + sl] > 0.f && s.exists(row, sl, aa);
            if (counted) {
                const float* x = s.xyz(row, sl);
                p = make_float4(x[0], x[1], x[2], __int_as_float(at));
                w = (long long)pts[2 * at] * a.q[aa * 14 + sl];
            }
        }
        const bool weighted = w != 0;
        const unsigned long long bal[2] = {__ballot(counted), __ballot(weighted)};
        int rank[2];
        block_rank<NW, 2>(bal, wcnt, rank, n);
        if (counted) k.ilist[rank[0]] = p;              // below N14: at most one entry per slot
        if (weighted) {
            k.jxyz[rank[1]] = p;
            k.jw[rank[1]] = w;
        }
    }
    if (tid == 0) {
        k.counts[0] = n[0];
        k.counts[1] = n[1];
    }
}

__global__ __launch_bounds__(NT) void dev_pair_kernel(const AbxDevelopabilityArgs a, void* ws, int chunk) {
    __shared__ float jx[J_CHUNK], jy[J_CHUNK], jz[J_CHUNK];
    __shared__ long long jw[J_CHUNK];
    const int b = blockIdx.y, tid = threadIdx.x;
    const Block k = block_of(ws, b, a.Lab);
    const int ni = k.counts[0], nj = k.counts[1];
    if ((int)blockIdx.x * NT >= ni) return;             // the whole workgroup: no barrier has been passed
    const int i = blockIdx.x * NT + tid;
    const bool mine = i < ni;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (mine) {
        const float4 p = k.ilist[i];
        xi = (double)p.x; yi = (double)p.y; zi = (double)p.z;
    }
    const double r2 = a.radius2;
    long long sap = 0;
    for (int j0 = 0; j0 < nj; j0 += chunk) {
        const int n = nj - j0 < chunk ? nj - j0 : chunk;
        __syncthreads();                                // the previous chunk has been walked
        for (int j = tid; j < n; j += NT) {
            const float4 p = k.jxyz[j0 + j];
            jx[j] = p.x; jy[j] = p.y; jz[j] = p.z;
            jw[j] = k.jw[j0 + j];
        }
        __syncthreads();
        if (mine)
            for (int j = 0; j < n; ++j) {
                const double dx = (double)jx[j] - xi, dy = (double)jy[j] - yi, dz = (double)jz[j] - zi;
                if ((dx * dx + dy * dy) + dz * dz <= r2) sap += jw[j];
            }
    }
    if (mine) k.sap[i] = sap;
}

__global__ __launch_bounds__(NT) void dev_reduce_kernel(const AbxDevelopabilityArgs a, void* ws) {
    __shared__ unsigned long long rsum[MAX_ROWS];       // sum of SAP_i of the row (two's complement)
    __shared__ int rn[MAX_ROWS];                        // its counted atoms
    __shared__ int info[MAX_ROWS];
    __shared__ unsigned long long tot[3];               // positive parts: all, CDR rows, region rows
    __shared__ int cnt[ABX_DEV_COLS];
    __shared__ double wmax[NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = a.L, Lab = a.Lab;
    const Structure s(a, b);
    const Block k = block_of(ws, b, Lab);
    const int ni = k.counts[0];
    const int* pts = a.points + (long long)b * L * 28;
    for (int r = tid; r < Lab; r += NT) {
        rsum[r] = 0ull;
        rn[r] = 0;
        info[r] = s.aatype(r) | (a.region && a.region[r] ? R_REGION : 0) | (is_cdr(a.cdr_def[r]) ? R_CDR : 0);
    }
    if (tid < 3) tot[tid] = 0ull;
    if (tid < ABX_DEV_COLS) cnt[tid] = 0;
    __syncthreads();
    // ---- the atoms: row sums, atom counts, positive parts
    {
        long long pa = 0, pc = 0, pr = 0;
        for (int i = tid; i < ni; i += NT) {
            const long long v = k.sap[i];
            const int row = __float_as_int(k.ilist[i].w) / 14, f = info[row];
            lds_add(&rsum[row], v);
            atomicAdd(&rn[row], 1);
            const long long p = v > 0 ? v : 0;
            pa += p;
            pc += (f & R_CDR) ? p : 0;
            pr += (f & R_REGION) ? p : 0;
        }
        lds_add(&tot[0], pa);
        lds_add(&tot[1], pc);
        lds_add(&tot[2], pr);
    }
    __syncthreads();
    // ---- the rows: presence, mean, charge, exposure
    const int heavy = a.chain_id[0];
    double best = -INFINITY;
    for (int r = tid; r < Lab; r += NT) {
        int f = info[r];
        const int aa = f & 31, n = rn[r];
        if (n == 0) continue;
        f |= R_PRESENT;
        const long long sum = (long long)rsum[r];
        const double mean = (double)sum / (double)n / FIXED_ONE;
        best = mean > best ? mean : best;
        if (sum > 0) {
            atomicAdd(&cnt[4], 1);
            if (f & R_REGION) atomicAdd(&cnt[5], 1);
        }
        const int ch = type_charge(aa);
        if (ch) atomicAdd(&cnt[a.chain_id[r] == heavy ? 6 : 7], ch);
        if (aa == T_HIS) atomicAdd(&cnt[9], 1);
        const double ref = a.ref[aa], rel = sidechain_rel_area(s, a.radius, pts, a.a, r, aa);
        if (aa == T_CYS && a.radius[aa * 14 + 5] > 0.f && s.exists(r, 5, aa)) f |= R_SG;
        if (row_exposed(rel, ref, a.exposed)) f |= R_EXPOSED;
        info[r] = f;
        if (a.rows) {
            double* o = a.rows + ((long long)b * L + r) * 4;
            o[0] = mean;
            o[1] = ref > 0.0 ? rel / ref : 0.0;
        }
    }
    best = wave_max_d(best);
    if (lane == 0) wmax[wv] = best;
    __syncthreads();
    // ---- links (both rows present)
    for (int r = tid + 1; r < Lab; r += NT)
        if ((info[r] & R_PRESENT) && (info[r - 1] & R_PRESENT) && linked_rows(a.chain_id, a.residx, r)) atomicOr(&info[r], R_LINK);
    __syncthreads();
    // ---- liabilities of the row that starts them
    for (int r = tid; r < L; r += NT) {
        int liab = 0, charge = 0;
        const int f = r < Lab ? info[r] : 0;
        if (f & R_PRESENT) {
            const int aa = f & 31;
            const bool ex = (f & R_EXPOSED) != 0;
            const int f1 = r + 1 < Lab ? info[r + 1] : 0, f2 = r + 2 < Lab ? info[r + 2] : 0;
            const bool l1 = (f1 & R_LINK) != 0, l2 = l1 && (f2 & R_LINK) != 0;
            const int a1 = f1 & 31, a2 = f2 & 31;
            if (ex && aa == T_ASN) {
                if (l2 && a1 != T_PRO && (a2 == T_SER || a2 == T_THR)) liab |= 1;
                if (l1 && (a1 == T_GLY || a1 == T_SER)) liab |= 2;
            }
            if (ex && aa == T_ASP) {
                if (l1 && (a1 == T_GLY || a1 == T_SER)) liab |= 4;
                if (l1 && a1 == T_PRO) liab |= 8;
            }
            if (ex && aa == T_MET) liab |= 16;
            if (ex && aa == T_TRP) liab |= 32;
            if (f & R_SG) {
                const float* x = s.xyz(r, 5);
                bool bonded = false;
                for (int o = 0; o < Lab; ++o) {
                    if (o == r || !(info[o] & R_SG)) continue;
                    const float* y = s.xyz(o, 5);
                    const double dx = (double)y[0] - (double)x[0], dy = (double)y[1] - (double)x[1], dz = (double)y[2] - (double)x[2];
                    if ((dx * dx + dy * dy) + dz * dz <= CYS_SS2) bonded = true;
                }
                if (!bonded) liab |= 64;
            }
            for (int c = 0; c < 7; ++c)
                if (liab >> c & 1) atomicAdd(&cnt[10 + c], 1);
            const int nl = __popc(liab);
            if (nl) {
                atomicAdd(&cnt[17], nl);
                if (f & R_REGION) atomicAdd(&cnt[18], nl);
                if (f & R_CDR) atomicAdd(&cnt[19], nl);
            }
            charge = type_charge(aa);
        }
        if (a.rows) {
            double* o = a.rows + ((long long)b * L + r) * 4;
            if (!(f & R_PRESENT)) o[0] = o[1] = 0.0;
            o[2] = (double)liab;
            o[3] = (double)charge;
        }
    }
    __syncthreads();
    if (tid < ABX_DEV_COLS) {
        double v;
        if (tid < 3) v = (double)(long long)tot[tid] / FIXED_ONE;
        else if (tid == 3) {
            v = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
            if (v == -INFINITY) v = 0.0;
        } else if (tid == 8) v = (double)cnt[6] * (double)cnt[7];
        else if (tid == 20) v = (double)ni;
        else v = (double)cnt[tid];
        a.out[(long long)b * a.out_stride + tid] = v;
    }
}

}  // namespace

extern "C" long long abx_developability_scores_workspace_bytes(int B, int L) {
    return B > 0 && L > 0 ? (long long)B * block_bytes(L) : 0;
}

extern "C" int abx_developability_scores(const AbxDevelopabilityArgs* ap, void* workspace, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_developability_scores: null");
    const AbxDevelopabilityArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_developability_scores", 1)) return rc;
    ABX_REQUIRE(a.chain_id && a.cdr_def && a.q && a.a && a.ref && a.points && a.out && workspace, "abx_developability_scores: null operand");
    ABX_REQUIRE(a.out_stride >= ABX_DEV_COLS, "abx_developability_scores: out_stride below ABX_DEV_COLS");
    ABX_REQUIRE(a.P >= 1 && a.P <= 1024, "abx_developability_scores: P must be in 1..1024");
    ABX_REQUIRE(std::isfinite(a.radius2) && a.radius2 > 0.0, "abx_developability_scores: radius2 must be > 0");
    ABX_REQUIRE(std::isfinite(a.exposed) && a.exposed >= 0.0 && a.exposed <= 1.0, "abx_developability_scores: exposed must be in [0, 1]");
    ABX_REQUIRE(a.j_chunk >= 0 && a.j_chunk <= J_CHUNK, "abx_developability_scores: j_chunk must be in 0..2048");
    ABX_REQUIRE(a.Lab <= MAX_ROWS, "abx_developability_scores: the row tables do not fit the LDS (Lab <= 2048)");
    ABX_REQUIRE(a.q_max >= 0 && 140.0 * (double)a.P * (double)a.q_max * (double)a.Lab * (double)a.Lab < 9.2e18,
                "abx_developability_scores: the sums could leave int64 (140 P q_max Lab^2 >= 2^63)");
    const int chunk = a.j_chunk ? a.j_chunk : J_CHUNK;
    // the workspace is laid out by Lab: the block of abx_developability_scores_workspace_bytes(B, L) holds it
    hipLaunchKernelGGL(dev_weigh_kernel, dim3(a.B), dim3(NT), 0, st, a, workspace);
    if (int rc = abx_check_launch("abx_developability_scores")) return rc;
    hipLaunchKernelGGL(dev_pair_kernel, dim3((a.Lab * 14 + NT - 1) / NT, a.B), dim3(NT), 0, st, a, workspace, chunk);
    if (int rc = abx_check_launch("abx_developability_scores")) return rc;
    hipLaunchKernelGGL(dev_reduce_kernel, dim3(a.B), dim3(NT), 0, st, a, workspace);
    return abx_check_launch("abx_developability_scores");
}
