// Design scores: the reference's offline evaluation of a written design - Kabsch-aligned C-alpha RMSD and amino-acid
// recovery per CDR (abx/common/ab_utils.py:124-167 calc_ab_metrics, abx/utils.py:444-465 kabsch_numpy), the violation masks of the
// peptide geometry (eval/metric_scripts/cal_vio.py:29-110) - plus the number of clashing atom pairs under the pair rules of the
// guidance clash energy (guidance.hip), computed where the sampler's records already are: one row of ABX_SCORE_COLS doubles per
// structure (include/abx_hip.h, AbxDesignScoreArgs).
//
// Two kernels, no atomics, every sum in a fixed order (a structure's row does not depend on its batch mates):
//   clash_count_kernel  grid (residue tile, structure), the O((14 L)^2) part, tiled like guidance.hip::clash_kernel: a block owns 16
//                       residues (224 atoms, one thread each) and streams its own tile and the following HALF of the tiles (cyclically)
//                       through LDS - every unordered pair is seen once, half the pair visits of the energy kernel, the same
//                       number of tiles in every block - and writes two integer partial counts.
//   score_row_kernel    one block per structure: centroids and the 3x3 covariance of the antibody C-alpha in fp64 (wave shuffles +
//                       a 4-entry LDS stage), Horn's quaternion form of the optimal proper rotation (thread 0: cyclic Jacobi on the
//                       4x4 symmetric matrix, both matrices in LDS so that no index is a register index), the per-region sums, the
//                       peptide violation counts (peptide_dev.h, shared with guidance.hip), the sum of the clash partials, the row.
#include "common.h"
#include "abx_hip.h"
#include "peptide_dev.h"
#include "reduce_dev.h"
#include "structure_dev.h"

namespace {

constexpr int RT = 16;                 // residues per tile
constexpr int AT = RT * 14;            // atoms per tile (224)

// The structure view (structure_dev.h) with what the peptide links need; the complex is shared by the batch or one per structure
struct Structure : StructureView<AbxDesignScoreArgs> {
    const int* chain; const int* residx;
    int L;
    __device__ __forceinline__ Structure(const AbxDesignScoreArgs& a, int b) : Structure(a, b, a.complex_batched ? (long long)b * a.L : 0) {}
    __device__ __forceinline__ Structure(const AbxDesignScoreArgs& a, int b, long long g) : StructureView<AbxDesignScoreArgs>(a, b, g) {
        chain = a.chain_id + g;
        residx = a.residx ? a.residx + g : nullptr;
        L = a.L;
    }
    __device__ __forceinline__ bool linked_to_prev(int res) const {
        return res > 0 && res < L && linked_rows(chain, residx, res);
    }
};

__global__ __launch_bounds__(256) void clash_count_kernel(const AbxDesignScoreArgs a, unsigned long long* __restrict__ part) {
    __shared__ float4 tile[AT];        // x, y, z, radius (radius < 0: atom absent)
    __shared__ int tag[AT];            // residue index << 6 | linked to predecessor << 5 | SG << 4 | atom slot
    __shared__ int chn[AT];            // chain id
    __shared__ int nred[4][2];
    const int b = blockIdx.y, it = blockIdx.x, tid = threadIdx.x, L = a.L;
    const Structure s(a, b);
    // the atom table entry of guidance.hip::clash_kernel
    auto load_atom = [&](int res, int slot, float4& p, int& t, int& c) {
        p = make_float4(0.f, 0.f, 0.f, -1.f);
        t = 0;
        c = 0;
        if (res < L) {
            const float* x = s.xyz(res, slot);
            const int aa = s.aatype(res);
            p = make_float4(x[0], x[1], x[2], s.exists(res, slot, aa) ? s.radius[aa * 14 + slot] : -1.f);
            // SG of cysteine sits in atom14 slot 5: flagged for the disulfide exclusion
            const int sg = (aa == 4 && slot == 5) ? 1 : 0;
            t = (res << 6) | ((s.linked_to_prev(res) ? 1 : 0) << 5) | (sg << 4) | slot;
            c = s.chain[res];
        }
    };
    const int mres = it * RT + tid / 14, mslot = tid % 14;
    float4 me = make_float4(0.f, 0.f, 0.f, -1.f);
    int mtag = 0, mchain = 0;
    if (tid < AT) load_atom(mres, mslot, me, mtag, mchain);
    const int msg = (mtag >> 4) & 1, mlink = (mtag >> 5) & 1;
    int n = 0, ninter = 0;
    // Tile pairs: a block takes its own tile, the next (nt - 1) / 2 tiles cyclically and - nt even - the opposite tile when it is the
    // lower of the two: every unordered pair of tiles once, and every block the same number of tiles (a triangular walk leaves the
    // first block with nt tiles while all blocks of a batch are resident at once: the longest block is the kernel's time)
    const int nt = (L + RT - 1) / RT;
    const int ntile = 1 + (nt - 1) / 2 + ((nt % 2 == 0 && it < nt / 2) ? 1 : 0);
    for (int st = 0; st < ntile; ++st) {
        const int jt = it + st < nt ? it + st : it + st - nt;
        __syncthreads();
        if (jt == it) {
            if (tid < AT) { tile[tid] = me; tag[tid] = mtag; chn[tid] = mchain; }
        } else if (tid < AT) {
            load_atom(jt * RT + tid / 14, tid % 14, tile[tid], tag[tid], chn[tid]);
        }
        __syncthreads();
        if (tid < AT && me.w > 0.f) {
            // own tile: the atoms after mine (the other residues among them); other tiles: all of them
            for (int k = jt == it ? tid + 1 : 0; k < AT; ++k) {
                const float4 o = tile[k];
                const int ot = tag[k];
                const int ores = ot >> 6;
                if (o.w <= 0.f || ores == mres) continue;
                const int oslot = ot & 15;
                // peptide bond C(i) - N(i+1) of linked neighbours, SG - SG disulfide
                if ((ores == mres + 1 && mslot == 2 && oslot == 0 && ((ot >> 5) & 1)) || (mres == ores + 1 && oslot == 2 && mslot == 0 && mlink)) continue;
                if (msg && ((ot >> 4) & 1)) continue;
                // the overlap of guidance.hip::clash_kernel, operation for operation
                const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
                const float d = sqrtf(1e-10f + dx * dx + dy * dy + dz * dz);
                const float ov = me.w + o.w - a.overlap_tolerance - d;
                if (ov > 0.f) {
                    ++n;
                    ninter += chn[k] != mchain ? 1 : 0;
                }
            }
        }
    }
    n = wave_sum_i(n);
    ninter = wave_sum_i(ninter);
    if ((tid & 63) == 0) { nred[tid >> 6][0] = n; nred[tid >> 6][1] = ninter; }
    __syncthreads();
    if (tid < 2) {
        unsigned long long v = 0;
        for (int w = 0; w < 4; ++w) v += (unsigned long long)nred[w][tid];
        part[((long long)b * gridDim.x + it) * 2 + tid] = v;
    }
}

constexpr int NREG = 7;                // heavy cdr1 / cdr2 / cdr3, light cdr1 / cdr2 / cdr3, heavy cdr3 Loop
__global__ __launch_bounds__(256) void score_row_kernel(const AbxDesignScoreArgs a, const unsigned long long* __restrict__ part, int nparts) {
    __shared__ double red[4 * 21];
    __shared__ double Nm[4][4], Vm[4][4];
    __shared__ double Rs[9];
    __shared__ int wcnt[4];
    const int b = blockIdx.x, tid = threadIdx.x, L = a.L, Lab = a.Lab;
    const Structure s(a, b);
    auto ca_ok = [&](int i) { return s.gexists[(long long)i * 14 + 1] != 0; };
    // ---- centroids of the C-alpha that take part, and the number of CDR-H3 rows
    double c0[8] = {0, 0, 0, 0, 0, 0, 0, 0};           // n, ground truth xyz, prediction xyz, CDR-H3 rows
    for (int i = tid; i < Lab; i += 256) {
        if (a.cdr_def[i] == 5) c0[7] += 1.0;
        if (!ca_ok(i)) continue;
        const float* g = s.gt + ((long long)i * 14 + 1) * 3;
        const float* p = s.xyz(i, 1);
        c0[0] += 1.0;
        c0[1] += (double)g[0]; c0[2] += (double)g[1]; c0[3] += (double)g[2];
        c0[4] += (double)p[0]; c0[5] += (double)p[1]; c0[6] += (double)p[2];
    }
    block_sum_d<8>(c0, red);
    const double cg[3] = {c0[1] / c0[0], c0[2] / c0[0], c0[3] / c0[0]};
    const double cp[3] = {c0[4] / c0[0], c0[5] / c0[0], c0[6] / c0[0]};
    const int nh3 = (int)c0[7];
    // ---- covariance S[j][k] = sum (g_j - cg_j)(p_k - cp_k): the ground truth is moved onto the prediction, as calc_ab_metrics does
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < Lab; i += 256) {
        if (!ca_ok(i)) continue;
        const float* g = s.gt + ((long long)i * 14 + 1) * 3;
        const float* p = s.xyz(i, 1);
        const double gx = (double)g[0] - cg[0], gy = (double)g[1] - cg[1], gz = (double)g[2] - cg[2];
        const double px = (double)p[0] - cp[0], py = (double)p[1] - cp[1], pz = (double)p[2] - cp[2];
        S[0] += gx * px; S[1] += gx * py; S[2] += gx * pz;
        S[3] += gy * px; S[4] += gy * py; S[5] += gy * pz;
        S[6] += gz * px; S[7] += gz * py; S[8] += gz * pz;
    }
    block_sum_d<9>(S, red);
    if (tid == 0) horn_rotation_lds(S, Nm, Vm, Rs);
    __syncthreads();
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rs[k];
    // ---- per region: sum |R (g - cg) - (p - cp)|^2, rows, equal tokens.  acc[r], acc[7 + r], acc[14 + r]
    double acc[3 * NREG];
#pragma unroll
    for (int k = 0; k < 3 * NREG; ++k) acc[k] = 0.0;
    int h3_before[1] = {0};                             // CDR-H3 rows in the chunks already walked
    for (int base = 0; base < Lab; base += 256) {
        const int i = base + tid;
        const int code = i < Lab ? a.cdr_def[i] : -1;
        // rank of this row among the CDR-H3 rows (sequence order, whatever their masks): the Loop slice is [4 : nh3 - 2]
        const unsigned long long bal[1] = {__ballot(code == 5)};
        int ranks[1];
        block_rank<4, 1>(bal, wcnt, ranks, h3_before);
        const int rank = ranks[0];
        if (i >= Lab || !ca_ok(i)) continue;
        const float* g = s.gt + ((long long)i * 14 + 1) * 3;
        const float* p = s.xyz(i, 1);
        const double gx = (double)g[0] - cg[0], gy = (double)g[1] - cg[1], gz = (double)g[2] - cg[2];
        const double ex = (R[0] * gx + R[1] * gy + R[2] * gz) - ((double)p[0] - cp[0]);
        const double ey = (R[3] * gx + R[4] * gy + R[5] * gz) - ((double)p[1] - cp[1]);
        const double ez = (R[6] * gx + R[7] * gy + R[8] * gz) - ((double)p[2] - cp[2]);
        const double d2 = ex * ex + ey * ey + ez * ez;
        const double same = s.pseq[i] == s.gseq[i] ? 1.0 : 0.0;
        const bool in_loop = code == 5 && rank >= 4 && rank < nh3 - 2;
        constexpr int CODE[6] = {1, 3, 5, 8, 10, 12};
#pragma unroll
        for (int r = 0; r < NREG; ++r) {
            const bool in = r < 6 ? code == CODE[r < 6 ? r : 0] : in_loop;
            acc[r] += in ? d2 : 0.0;
            acc[NREG + r] += in ? 1.0 : 0.0;
            acc[2 * NREG + r] += in ? same : 0.0;
        }
    }
    block_sum_d<3 * NREG>(acc, red);
    // ---- peptide violations of the pairs (l, l + 1): the three masks of cal_vio.py, counted
    int nv[3] = {0, 0, 0};
    for (int l = tid; l < L - 1; l += 256) {
        if (!s.linked_to_prev(l + 1)) continue;
        const int aa_l = s.aatype(l), aa_u = s.aatype(l + 1);
        if (!s.exists(l, 2, aa_l) || !s.exists(l + 1, 0, aa_u)) continue;
        PairGrad o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.g[k][0] = o.g[k][1] = o.g[k][2] = 0.f;
        o.eb = o.ea = 0.f;
        o.viol = 0;
        peptide_terms(s.xyz(l, 1), s.xyz(l, 2), s.xyz(l + 1, 0), s.xyz(l + 1, 1), s.exists(l, 1, aa_l), s.exists(l + 1, 1, aa_u),
                      aa_u == 14, 1.0f, 1.0f, a.bond_tolerance_factor, o);
        nv[0] += o.viol & 1;
        nv[1] += (o.viol >> 1) & 1;
        nv[2] += (o.viol >> 2) & 1;
    }
    double vio[3] = {(double)nv[0], (double)nv[1], (double)nv[2]};
    block_sum_d<3>(vio, red);
    if (tid == 0) {
        double* out = a.out + (long long)b * a.out_stride;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        // columns: region r -> (AAR, RMSD); heavy cdr3 and its Loop interleave as AAR, Loop AAR, RMSD, Loop RMSD
        constexpr int COL_AAR[NREG] = {0, 2, 4, 8, 10, 12, 5};
        constexpr int COL_RMSD[NREG] = {1, 3, 6, 9, 11, 13, 7};
#pragma unroll
        for (int r = 0; r < NREG; ++r) {
            const double n = acc[NREG + r];
            out[COL_AAR[r]] = n > 0.0 ? acc[2 * NREG + r] / n : nan;
            out[COL_RMSD[r]] = n > 0.0 ? sqrt(acc[r] / n) : nan;
        }
        out[14] = vio[0]; out[15] = vio[1]; out[16] = vio[2];
        unsigned long long nc = 0, ni = 0;
        for (int k = 0; k < nparts; ++k) {
            nc += part[((long long)b * nparts + k) * 2];
            ni += part[((long long)b * nparts + k) * 2 + 1];
        }
        out[17] = (double)nc;
        out[18] = (double)ni;
    }
}

}  // namespace

extern "C" long long abx_design_scores_workspace_bytes(int B, int L) {
    if (B <= 0 || L <= 0) return 0;
    return (long long)B * ((L + RT - 1) / RT) * 2 * sizeof(unsigned long long);
}

extern "C" int abx_design_scores(const AbxDesignScoreArgs* ap, void* workspace, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_design_scores: null");
    const AbxDesignScoreArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_design_scores", 2)) return rc;
    ABX_REQUIRE(a.cdr_def && a.chain_id && a.out, "abx_design_scores: null operand");
    ABX_REQUIRE(a.out_stride >= ABX_SCORE_COLS, "abx_design_scores: out_stride below ABX_SCORE_COLS");
    ABX_REQUIRE(workspace != nullptr, "abx_design_scores: null workspace");
    const int nparts = (a.L + RT - 1) / RT;
    unsigned long long* part = reinterpret_cast<unsigned long long*>(workspace);
    hipLaunchKernelGGL(clash_count_kernel, dim3(nparts, a.B), dim3(256), 0, st, a, part);
    int rc = abx_check_launch("abx_design_scores(clash count)");
    if (rc) return rc;
    hipLaunchKernelGGL(score_row_kernel, dim3(a.B), dim3(256), 0, st, a, part, nparts);
    return abx_check_launch("abx_design_scores");
}
