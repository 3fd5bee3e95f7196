// Torsion analysis of designs (include/abx_hip.h, AbxTorsionArgs): phi, psi and omega between the residues - cis and twisted peptides,
// phi >= 0, the ABEGO class - and the chi angles against the crystal structure.  One row of ABX_TORSION_COLS doubles per structure.
//
// One kernel, one workgroup of 256 per structure, one lane per antibody row (strided), two passes over the same code:
//   wild type  N, CA, C of every row staged as float64 in LDS (9 doubles a row: lanes 18 dwords apart, no bank is hit twice by a
//              64-bit read of a half wave); the (x, y) pair of every dihedral of a row and its code go to the workspace;
//   design     staged over the same LDS, measured the same way and compared with the row's own words of the workspace - written and
//              read back by the same lane, so no fence is needed and a workgroup touches nothing but its own slice.
// Every decision is taken on (x, y): products, one square root and a comparison, in float64 without fused multiply-add; atan2 only
// reports.  Counts: integer LDS adds (they commute).  The thresholds' cosines, the residue types and the region flags sit in LDS beside
// the backbone: the kernel keeps no scalar register spilled.  The four float sums: block_sum_d (fixed order).  The maximum: an
// integer LDS maximum of the bit pattern of a non-negative double.  A structure's row does not depend on its batch mates.
#include "common.h"
#include "abx_hip.h"
#include "peptide_dev.h"
#include "reduce_dev.h"
#include "structure_dev.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int WS = 16;                  // doubles per row in the workspace: (x, y) of phi, psi, omega, chi1..chi4, the word, one spare
constexpr int NC = 24;                  // integer counters
constexpr double DEG = 57.29577951308232;       // 180 / pi
// the word of a row: bit 0 phi, 1 psi, 2 omega, 3..6 chi1..chi4 defined; bits 8..10 the ABEGO code
constexpr int HAS_PHI = 1, HAS_PSI = 2, HAS_OMEGA = 4, HAS_CHI = 8, CODE_SHIFT = 8;
constexpr int F_CIS = 8, F_TWISTED = 16, F_PHI_POS = 32, F_REGION = 64, F_CHI1 = 128, F_CHI1_OK = 256;

struct Dih { double x, y; };

__device__ __forceinline__ Dih dihedral(const double* a, const double* b, const double* c, const double* d) {
    const double b1x = b[0] - a[0], b1y = b[1] - a[1], b1z = b[2] - a[2];
    const double b2x = c[0] - b[0], b2y = c[1] - b[1], b2z = c[2] - b[2];
    const double b3x = d[0] - c[0], b3y = d[1] - c[1], b3z = d[2] - c[2];
    const double n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
    const double n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
    Dih r;
    r.x = (n1x * n2x + n1y * n2y) + n1z * n2z;
    r.y = sqrt((b2x * b2x + b2y * b2y) + b2z * b2z) * ((b1x * n2x + b1y * n2y) + b1z * n2z);
    return r;
}

__device__ __forceinline__ double radius_of(const Dih& t) { return sqrt(t.x * t.x + t.y * t.y); }
__device__ __forceinline__ double degrees_of(const Dih& t) { return atan2(t.y, t.x) * DEG; }

__global__ __launch_bounds__(256) void torsion_kernel(const AbxTorsionArgs a, double* __restrict__ wsp) {
    extern __shared__ double bb[];                      // [Lab][9]: N, CA, C of the staged structure
    __shared__ unsigned char have[ABX_TORSION_MAX_LAB]; // N, CA and C of the row of the staged structure are present
    __shared__ unsigned char typ[2][ABX_TORSION_MAX_LAB];       // the residue type of the row in the design [0] and in the wild type [1]
    __shared__ unsigned char regs[ABX_TORSION_MAX_LAB]; // the row is a region row
    __shared__ int cnt[NC];
    __shared__ unsigned long long dmax;
    __shared__ double red[4 * 4];
    __shared__ double th[8];                            // cos of cis, trans, o, a_half, g_half, chi_tol; (cos, sin) of a_mid
    const int b = blockIdx.x, tid = threadIdx.x, Lab = a.Lab;
    const StructureView<AbxTorsionArgs> s(a, b);
    double* ws = wsp + (long long)b * Lab * WS;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    auto type_of = [&](int i, bool wild) { return wild ? s.clamp_aa(s.gseq[i]) : s.aatype(i); };
    auto present = [&](int i, int slot, int aa, bool wild) {
        return wild ? (s.kept(i) && s.gexists[(long long)i * 14 + slot] != 0) : s.exists(i, slot, aa);
    };
    auto atom = [&](int i, int slot, bool wild) { return (wild ? s.gt : s.pred) + ((long long)i * 14 + slot) * 3; };      // (rows < Lab <= Lpred)
    auto stage = [&](bool wild) {
        for (int i = tid; i < Lab; i += 256) {
            const int aa = type_of(i, wild);
            bool all = true;
#pragma unroll
            for (int slot = 0; slot < 3; ++slot) {
                const float* p = atom(i, slot, wild);
                all = all && present(i, slot, aa, wild);
                bb[i * 9 + slot * 3 + 0] = (double)p[0];
                bb[i * 9 + slot * 3 + 1] = (double)p[1];
                bb[i * 9 + slot * 3 + 2] = (double)p[2];
            }
            have[i] = all ? 1 : 0;
            typ[wild ? 1 : 0][i] = (unsigned char)aa;
            regs[i] = (a.region && a.region[i] && s.kept(i)) ? 1 : 0;
        }
    };
    auto link = [&](int i) { return i >= 1 && i < Lab && have[i - 1] && have[i] && linked_rows(a.chain_id, a.residx, i); };
    // the seven (x, y) pairs of row i of the staged structure -> the defined bits
    auto measure = [&](int i, bool wild, Dih (&t)[7]) {
        int bits = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) t[k].x = t[k].y = 0.0;
        const double* m = bb + i * 9;
        if (link(i)) {
            t[0] = dihedral(m - 3, m, m + 3, m + 6);                    // C' N CA C
            t[2] = dihedral(m - 6, m - 3, m, m + 3);                    // CA' C' N CA
            bits |= HAS_PHI | HAS_OMEGA;
        }
        if (link(i + 1)) {
            t[1] = dihedral(m, m + 3, m + 6, m + 9);                    // N CA C N"
            bits |= HAS_PSI;
        }
        const int aa = typ[wild ? 1 : 0][i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int* sl = a.chi_atoms + aa * 16 + k * 4;
            int q[4];
            bool ok = true;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                q[j] = sl[j];
                ok = ok && q[j] >= 0 && q[j] < 14 && present(i, q[j], aa, wild);
            }
            if (!ok) continue;
            double p[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* f = atom(i, q[j], wild);
                p[j][0] = (double)f[0]; p[j][1] = (double)f[1]; p[j][2] = (double)f[2];
            }
            t[3 + k] = dihedral(p[0], p[1], p[2], p[3]);
            bits |= HAS_CHI << k;
        }
        return bits;
    };
    auto code_of = [&](int bits, const Dih (&t)[7]) {
        if ((bits & 7) != 7) return 0;
        const double ro = radius_of(t[2]), rp = radius_of(t[1]);
        if (!(t[2].x <= th[2] * ro)) return 5;
        if (t[0].y < 0.0) return (t[1].x * th[6] + t[1].y * th[7] >= th[3] * rp) ? 1 : 2;
        return (t[1].x >= th[4] * rp) ? 3 : 4;
    };

    if (tid < NC) cnt[tid] = 0;
    if (tid == 0) {
        dmax = 0ull;
        th[0] = a.cis[0]; th[1] = a.trans[0]; th[2] = a.o[0]; th[3] = a.a_half[0]; th[4] = a.g_half[0]; th[5] = a.chi_tol[0];
        th[6] = a.a_mid[0]; th[7] = a.a_mid[1];
    }
    auto count = [&](int k, int n) { if (n) atomicAdd(&cnt[k], n); };
    double v[4] = {0.0, 0.0, 0.0, 0.0};                 // sums of |delta phi|, |delta psi|, |delta omega|, |delta chi|
    double big = 0.0;
    // ---- the wild type, to the workspace
    stage(true);
    __syncthreads();
    for (int i = tid; i < Lab; i += 256) {
        Dih t[7];
        const int bits = measure(i, true, t);
        double* w = ws + (long long)i * WS;
#pragma unroll
        for (int k = 0; k < 7; ++k) { w[2 * k] = t[k].x; w[2 * k + 1] = t[k].y; }
        w[14] = __longlong_as_double((long long)(bits | (code_of(bits, t) << CODE_SHIFT)));
        w[15] = 0.0;
    }
    __syncthreads();                                    // every lane has read the wild type's rows
    // ---- the design, against it
    stage(false);
    __syncthreads();
    for (int i = tid; i < Lab; i += 256) {
        Dih t[7], g[7];
        const int bits = measure(i, false, t);
        const int code = code_of(bits, t);
        const double* w = ws + (long long)i * WS;
#pragma unroll
        for (int k = 0; k < 7; ++k) { g[k].x = w[2 * k]; g[k].y = w[2 * k + 1]; }
        const int wword = (int)__double_as_longlong(w[14]);
        const int wbits = wword & 0xff, wcode = wword >> CODE_SHIFT;
        const int aa = typ[0][i];
        const bool reg = regs[i] != 0;
        const bool reg_link = reg || (i >= 1 && regs[i - 1] != 0);
        int flags = code | (reg ? F_REGION : 0);
        if (bits & HAS_OMEGA) {
            const double ro = radius_of(t[2]);
            const bool wide = t[2].x <= th[0] * ro;
            const int cis = wide ? 0 : 1, tw = (wide && !(t[2].x <= th[1] * ro)) ? 1 : 0;
            const int rl = reg_link ? 1 : 0;
            count(0, 1); count(1, cis); count(2, (cis && aa != a.pro) ? 1 : 0); count(3, tw);
            count(4, rl); count(5, cis & rl); count(6, tw & rl);
            flags |= (cis ? F_CIS : 0) | (tw ? F_TWISTED : 0);
        }
        if ((bits & HAS_PHI) && !(t[0].y < 0.0) && aa != a.gly) {
            count(7, 1); count(8, reg ? 1 : 0);
            flags |= F_PHI_POS;
        }
        // |delta| of pair k against the wild type's, in degrees; fold: modulo 180
        auto delta = [&](int k, bool fold, bool& ok) {
            double cc = t[k].x * g[k].x + t[k].y * g[k].y;
            const double ss = t[k].y * g[k].x - t[k].x * g[k].y;
            if (fold) cc = fabs(cc);
            ok = cc >= th[5] * sqrt(cc * cc + ss * ss);
            return atan2(fabs(ss), cc) * DEG;
        };
        if (reg) {
            count(9, code == 1 ? 1 : 0); count(10, code == 2 ? 1 : 0); count(11, code == 3 ? 1 : 0); count(12, code == 4 ? 1 : 0); count(13, code == 5 ? 1 : 0);
            if (code && wcode) { count(14, 1); count(15, code == wcode ? 1 : 0); }
            bool ok;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (bits & wbits & (1 << k)) {
                    const double d = delta(k, false, ok);
                    v[k] += d; count(16 + k, 1);
                    if (k < 2) big = d > big ? d : big;
                }
            if (aa == typ[1][i]) {
                bool ok1 = false, ok2 = false;
                const int both = bits & wbits;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (both & (HAS_CHI << k)) {
                        const double d = delta(3 + k, a.chi_pi[aa * 4 + k] != 0, ok);
                        v[3] += d; count(23, 1);
                        if (k == 0) ok1 = ok;
                        if (k == 1) ok2 = ok;
                    }
                if (both & HAS_CHI) {
                    count(19, 1); count(20, ok1 ? 1 : 0);
                    flags |= F_CHI1 | (ok1 ? F_CHI1_OK : 0);
                    if (both & (HAS_CHI << 1)) { count(21, 1); count(22, (ok1 && ok2) ? 1 : 0); }
                }
            }
        }
        if (a.rows) {
            double* dst = a.rows + ((long long)b * Lab + i) * 8;
#pragma unroll
            for (int k = 0; k < 7; ++k) dst[k] = (bits & (1 << k)) ? degrees_of(t[k]) : nan;
            dst[7] = (double)flags;
        }
        if (a.classes) a.classes[(long long)b * Lab + i] = code;
    }
    if (big > 0.0) atomicMax(&dmax, (unsigned long long)__double_as_longlong(big));
    block_sum_d<4>(v, red);                             // (its barriers also order the counters before the read below)
    if (tid == 0) {
        double* out = a.out + (long long)b * a.out_stride;
#pragma unroll
        for (int k = 0; k < 16; ++k) out[k] = (double)cnt[k];
        auto mean = [&](double sum, int n) { return n > 0 ? sum / (double)n : nan; };
        out[16] = mean(v[0], cnt[16]);
        out[17] = mean(v[1], cnt[17]);
        out[18] = mean(v[2], cnt[18]);
        out[19] = (cnt[16] + cnt[17]) > 0 ? __longlong_as_double((long long)dmax) : nan;
        out[20] = (double)cnt[19]; out[21] = (double)cnt[20]; out[22] = (double)cnt[21]; out[23] = (double)cnt[22];
        out[24] = mean(v[3], cnt[23]);
    }
}

bool unit_pair(const double* p) {
    return std::isfinite(p[0]) && std::isfinite(p[1]) && std::fabs(p[0] * p[0] + p[1] * p[1] - 1.0) <= 1e-9;
}

}  // namespace

extern "C" long long abx_torsion_scores_workspace_bytes(int B, int Lab) {
    if (B <= 0 || Lab <= 0) return 0;
    return (long long)B * Lab * WS * sizeof(double);
}

extern "C" int abx_torsion_scores(const AbxTorsionArgs* ap, void* workspace, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_torsion_scores: null");
    const AbxTorsionArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_torsion_scores", 1)) return rc;
    ABX_REQUIRE(a.out && a.chain_id && a.chi_atoms && a.chi_pi, "abx_torsion_scores: null operand");
    ABX_REQUIRE(a.out_stride >= ABX_TORSION_COLS, "abx_torsion_scores: out_stride below ABX_TORSION_COLS");
    ABX_REQUIRE(a.Lab <= ABX_TORSION_MAX_LAB, "abx_torsion_scores: Lab <= 800 (ABX_TORSION_MAX_LAB: the backbone of a structure is staged in LDS)");
    ABX_REQUIRE(unit_pair(a.cis) && unit_pair(a.trans) && unit_pair(a.o) && unit_pair(a.a_mid) && unit_pair(a.a_half) && unit_pair(a.g_half) &&
                unit_pair(a.chi_tol), "abx_torsion_scores: every threshold must be a (cos, sin) pair");
    ABX_REQUIRE(a.gly >= 0 && a.gly <= 20 && a.pro >= 0 && a.pro <= 20, "abx_torsion_scores: gly and pro must be residue types 0..20");
    ABX_REQUIRE(workspace != nullptr, "abx_torsion_scores: null workspace");
    hipLaunchKernelGGL(torsion_kernel, dim3(a.B), dim3(256), (size_t)a.Lab * 9 * sizeof(double), st, a, reinterpret_cast<double*>(workspace));
    return abx_check_launch("abx_torsion_scores");
}
