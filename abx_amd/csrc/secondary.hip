// Secondary structure of designs (include/abx_hip.h, AbxSecondaryArgs): DSSP's electrostatic backbone hydrogen bonds on a virtual H over
// the antibody rows, and from them turns, helices, bridges, ladders and bends, against the crystal structure.  One row of
// ABX_SECONDARY_COLS doubles per structure.
//
// One kernel, one workgroup of 256 per structure, two passes over the same code - the wild type first, then the design against it:
//   stage     N, CA, C, O of every row as float32 in LDS (12 floats a row; the widening to float64 at the use is exact);
//   energy    one lane per donor (strided): its N, CA and virtual H stay in float64 registers - no other lane reads an H, so it is not
//             staged.  Per word of 32 acceptors first the CA prefilter of all of them, at lane-uniform LDS addresses (a broadcast, no
//             bank conflict) and without a branch, into a candidate mask; then every lane walks the set bits of its OWN mask through the
//             four-distance energy, so a wave runs the expensive body max-popcount times per word, not once for every acceptor that
//             is near ANY of its 64 donors.  These second reads are per lane, rows 12 dwords apart: some bank conflict is expected
//             and has not been measured.
//             The bonds of donor i are the bits of row i of the LDS matrix bm[Lab][W], W = ceil(Lab / 32) | 1 (an odd row stride:
//             the word stores of a wave spread over the banks); a row is written by its own lane alone, one plain store per word,
//             so neither an atomic OR nor a cleared matrix is needed.  Bonds accepted: an LDS atomic add per bond (sparse).
//   patterns  one lane per row between barriers, bit tests on bm: turns, bends, bridges and ladders (the candidates of row i are the
//             set bits of rows i and i + 1 and their right neighbours, walked in ascending order); H and E / B; G; I; T, S and the rest.
//             A lane that tests a neighbour's state tests membership in the set of EARLIER priorities only, which the lanes of the
//             same phase never write.
// The wild type's bit image (Lab * W words) and one word per row (state | present | CONT(i-1, i+1)) go to this workgroup's slice of
// the workspace.  The design pass reads them from lanes other than the writers (the bridge test of a pair reads rows i-1 .. j+1):
// every such read lies behind the __syncthreads() that ends the wild pass - a workgroup barrier with the workgroup-scope release /
// acquire fence, and all waves of a workgroup share one vector L1 - and no lane reads a word of the slice before that barrier, so an
// uninitialised workspace is never seen.  Counts: integer LDS adds (they commute); the energy: rint(e * 2^20) into a 64-bit LDS
// integer.  A structure's row does not depend on its batch mates.
#include "common.h"
#include "abx_hip.h"
#include "peptide_dev.h"
#include "structure_dev.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int MAXL = ABX_SECONDARY_MAX_LAB;
constexpr int NC = 24;                                  // integer counters: counter k is column k of the row; slot 5 stays 0 and unused
                                                        // (column 5, the energy, is the 64-bit sum esum), 22 and 23 are spare
constexpr double COULOMB = 27.888, CA_CUTOFF2 = 81.0, MIN_DIST = 0.5, MIN_ENERGY = -9.9, FIXED = 1048576.0;
// the pattern word of a row
constexpr int P_T3 = 1, P_T4 = 2, P_T5 = 4, P_BEND = 8, P_PAR = 16, P_ANTI = 32, P_LAD = 64;
// the word of a wild-type row in the workspace: its state in the low byte
constexpr unsigned W_PRESENT = 256, W_CONT3 = 512;
constexpr int F_REGION = 1, F_PRESENT = 2, F_HAS_H = 4, F_PARALLEL = 8, F_ANTIPARALLEL = 16, F_BEND = 32, F_TURN3 = 64;

__host__ __device__ constexpr int words_of(int Lab) { return ((Lab + 31) >> 5) | 1; }
__host__ __device__ constexpr long long slice_words(int Lab) { return (long long)Lab * (words_of(Lab) + 1); }
constexpr int LDS_MAX = MAXL * 12 * 4 + MAXL * words_of(MAXL) * 4;

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }
__device__ __forceinline__ int class3(int state) { return state == 0 ? 0 : (state <= 3 ? 1 : (state <= 5 ? 2 : 3)); }

__global__ __launch_bounds__(256) void secondary_kernel(const AbxSecondaryArgs a, unsigned* __restrict__ wsp) {
    extern __shared__ float dyn[];                      // xyz[Lab][12]: N, CA, C, O of the staged structure; then bm[Lab][W]
    __shared__ unsigned char have[MAXL];                // the row of the staged structure is present
    __shared__ unsigned char lnk[MAXL];                 // the link (i-1, i) of the staged structure
    __shared__ unsigned char hasH[MAXL];                // staging: the type is not pro; after the energy phase: the row has an H
    __shared__ unsigned char regs[MAXL];                // the row is a region row
    __shared__ unsigned char st[MAXL];                  // the state of the row
    __shared__ unsigned short don[MAXL];                // bonds donated
    __shared__ int acc[MAXL];                           // bonds accepted
    __shared__ int pat[MAXL];                           // the pattern word
    __shared__ short2 part[MAXL];                       // the lowest and the next bridge partner row, -1: none
    __shared__ int cnt[NC];
    __shared__ unsigned long long esum;
    __shared__ int* rows_p;                             // rows, classes, chain_id, residx of the arguments: read after the first barrier, and kept
    __shared__ int* classes_p;                          // here so that the kernel keeps no scalar register spilled
    __shared__ const int* chain_p;
    __shared__ const int* residx_p;
    __shared__ double th[2];                            // hb_energy, cos of the bend angle: in LDS, not in scalar registers
    const int b = blockIdx.x, tid = threadIdx.x, Lab = a.Lab, W = words_of(Lab);
    const StructureView<AbxSecondaryArgs> s(a, b);
    float* xyz = dyn;
    unsigned* bm = reinterpret_cast<unsigned*>(dyn + Lab * 12);
    unsigned* ws = wsp + (long long)b * slice_words(Lab);       // the wild type's image [Lab][W]
    unsigned* wword = ws + (long long)Lab * W;                  // ... and its row words [Lab]

    auto bit = [&](int d, int ac) { return (bm[d * W + (ac >> 5)] >> (ac & 31)) & 1u; };                       // hb(ac -> d) of the staged structure
    auto wbit = [&](int d, int ac) { return (ws[(long long)d * W + (ac >> 5)] >> (ac & 31)) & 1u; };           // ... of the wild type
    auto cont3 = [&](int i) { return (i >= 1 && i <= Lab - 2) ? (unsigned)(lnk[i] & lnk[i + 1]) : 0u; };
    auto wcont3 = [&](int i) { return (wword[i] >> 9) & 1u; };                                                  // (W_CONT3)
    auto cont = [&](int lo, int hi) {
        if (lo < 0 || hi >= Lab) return false;
        unsigned ok = 1u;
        for (int k = lo + 1; k <= hi; ++k) ok &= lnk[k];
        return ok != 0u;
    };
    // BRIDGE(i, j) of one type from a bond accessor f(donor, acceptor) and a CONT(i-1, i+1) accessor, both 0 / 1: one range branch, then
    // bit arithmetic without further branches
    auto bridge_of = [&](auto f, auto c3, int i, int j, bool anti) {
        const int d = i > j ? i - j : j - i;
        if (i < 1 || j < 1 || i > Lab - 2 || j > Lab - 2 || d < 3) return false;
        const unsigned r = anti ? ((f(j, i) & f(i, j)) | (f(j + 1, i - 1) & f(i + 1, j - 1)))
                                : ((f(j, i - 1) & f(i + 1, j)) | (f(i, j - 1) & f(j + 1, i)));
        return (r & c3(i) & c3(j)) != 0u;
    };
    auto count = [&](int k, int n) { if (n) atomicAdd(&cnt[k], n); };

    if (tid < NC) cnt[tid] = 0;
    if (tid == 0) { esum = 0ull; th[0] = a.hb_energy; th[1] = a.bend[0]; rows_p = a.rows; classes_p = a.classes; chain_p = a.chain_id; residx_p = a.residx; }

    auto pass = [&](const bool wild) {
        // ---- stage
        // (rows < Lab <= Lpred: the conventions of StructureView for a predicted row, with the pointers of this pass chosen once)
        const float* src = wild ? s.gt : s.pred;
        const long long* sq = wild ? s.gseq : s.pseq;
        const unsigned char* mk = wild ? s.gexists : s.pmask;
        for (int i = tid; i < Lab; i += 256) {
            const int aa = s.clamp_aa(sq[i]);
            const bool kept = s.kept(i);
            bool all = kept;
#pragma unroll
            for (int slot = 0; slot < 4; ++slot) {
                const float* p = src + ((long long)i * 14 + slot) * 3;
                all = all && (mk ? mk[(long long)i * 14 + slot] != 0 : s.radius[aa * 14 + slot] > 0.f);
                xyz[i * 12 + slot * 3 + 0] = p[0];
                xyz[i * 12 + slot * 3 + 1] = p[1];
                xyz[i * 12 + slot * 3 + 2] = p[2];
            }
            have[i] = all ? 1 : 0;
            hasH[i] = aa != a.pro ? 1 : 0;
            regs[i] = (a.region && a.region[i] && kept) ? 1 : 0;
            acc[i] = 0;
        }
        __syncthreads();
        // ---- energy: one lane per donor
        int n_hb = 0, n_reg = 0, n_in = 0, n_kept = 0;
        long long efix = 0;
        for (int i = tid; i < Lab; i += 256) {
            const bool li = i >= 1 && have[i - 1] && have[i] && linked_rows(chain_p, residx_p, i);
            bool h = li && hasH[i];
            const float* m = xyz + i * 12;
            const double Nx = (double)m[0], Ny = (double)m[1], Nz = (double)m[2], Ax = (double)m[3], Ay = (double)m[4], Az = (double)m[5];
            double Hx = 0.0, Hy = 0.0, Hz = 0.0;
            if (h) {
                const double vx = (double)m[-6] - (double)m[-3], vy = (double)m[-5] - (double)m[-2], vz = (double)m[-4] - (double)m[-1];     // C - O of row i-1
                const double n = norm3(vx, vy, vz);
                if (n == 0.0) h = false;
                else { Hx = Nx + vx / n; Hy = Ny + vy / n; Hz = Nz + vz / n; }
            }
            const bool ri = regs[i] != 0;
            int donated = 0;
            for (int w = 0; w < W; ++w) {                // (every word of the row is stored, the spare ones as 0)
                unsigned word = 0u;
                if (h) {
                    // the C-alpha prefilter of the 32 acceptors of this word: lane-uniform addresses, no branch
                    unsigned cand = 0u;
                    const int j1 = min(Lab, (w + 1) * 32);
                    for (int j = w * 32; j < j1; ++j) {
                        const float* q = xyz + j * 12 + 3;
                        const double dx = Ax - (double)q[0], dy = Ay - (double)q[1], dz = Az - (double)q[2];
                        const bool ok = have[j] && j != i && j != i - 1 && (dx * dx + dy * dy) + dz * dz < CA_CUTOFF2;      // (an H implies the link
                        cand |= (ok ? 1u : 0u) << (j & 31);                                                                 // (i-1, i): the own peptide bond is skipped)
                    }
                    // the wild type's word of the same donor: written by this lane in the wild pass
                    const unsigned wildw = (!wild && cand) ? ws[(long long)i * W + w] : 0u;
                    // the energy of the acceptors that passed: each lane walks its own
                    while (cand) {
                        const int j = w * 32 + __ffs(cand) - 1;
                        cand &= cand - 1u;
                        const float* q = xyz + j * 12;
                        const double Cx = (double)q[6], Cy = (double)q[7], Cz = (double)q[8], Ox = (double)q[9], Oy = (double)q[10], Oz = (double)q[11];
                        const double d_no = norm3(Nx - Ox, Ny - Oy, Nz - Oz), d_hc = norm3(Hx - Cx, Hy - Cy, Hz - Cz);
                        const double d_ho = norm3(Hx - Ox, Hy - Oy, Hz - Oz), d_nc = norm3(Nx - Cx, Ny - Cy, Nz - Cz);
                        double e = COULOMB * (((1.0 / d_no + 1.0 / d_hc) - 1.0 / d_ho) - 1.0 / d_nc);
                        if (d_no < MIN_DIST || d_hc < MIN_DIST || d_ho < MIN_DIST || d_nc < MIN_DIST) e = MIN_ENERGY;
                        if (e < th[0]) {
                            word |= 1u << (j & 31);
                            ++donated;
                            atomicAdd(&acc[j], 1);
                            const bool rj = regs[j] != 0;
                            ++n_hb;
                            if (ri || rj) { ++n_reg; efix += llrint(e * FIXED); n_kept += (int)((wildw >> (j & 31)) & 1u); }
                            if (ri && rj) ++n_in;
                        }
                    }
                }
                bm[i * W + w] = word;
                if (wild) ws[(long long)i * W + w] = word;
            }
            lnk[i] = li ? 1 : 0;
            hasH[i] = h ? 1 : 0;
            don[i] = (unsigned short)donated;
        }
        if (wild) count(3, n_reg);
        else {
            count(0, n_hb); count(1, n_reg); count(2, n_in); count(4, n_kept);
            if (efix) atomicAdd(&esum, (unsigned long long)efix);
        }
        __syncthreads();
        // ---- turns, bends, bridges and ladders
        int n_bridge = 0, n_bkept = 0;
        for (int i = tid; i < Lab; i += 256) {
            int p = 0;
#pragma unroll
            for (int n = 3; n <= 5; ++n)
                if (i + n < Lab && cont(i, i + n) && bit(i + n, i)) p |= P_T3 << (n - 3);
            if (cont(i - 2, i + 2)) {
                const float *c0 = xyz + (i - 2) * 12 + 3, *c1 = xyz + i * 12 + 3, *c2 = xyz + (i + 2) * 12 + 3;
                const double ux = (double)c1[0] - (double)c0[0], uy = (double)c1[1] - (double)c0[1], uz = (double)c1[2] - (double)c0[2];
                const double vx = (double)c2[0] - (double)c1[0], vy = (double)c2[1] - (double)c1[1], vz = (double)c2[2] - (double)c1[2];
                const double c = (ux * vx + uy * vy) + uz * vz;
                if (c < th[1] * (norm3(ux, uy, uz) * norm3(vx, vy, vz))) p |= P_BEND;
            }
            int p0 = -1, p1 = -1;
            if (cont3(i)) {
                unsigned carry = 0u;
                for (int w = 0; w < W; ++w) {
                    const unsigned c = bm[i * W + w] | bm[(i + 1) * W + w];
                    unsigned cand = c | (c << 1) | carry;
                    carry = c >> 31;
                    while (cand) {
                        const int j = w * 32 + __ffs(cand) - 1;
                        cand &= cand - 1u;
                        const bool par = bridge_of(bit, cont3, i, j, false), anti = bridge_of(bit, cont3, i, j, true);
                        if (!(par || anti)) continue;
                        if (p0 < 0) p0 = j; else if (p1 < 0) p1 = j;
                        p |= (par ? P_PAR : 0) | (anti ? P_ANTI : 0);
                        if ((par && (bridge_of(bit, cont3, i + 1, j + 1, false) || bridge_of(bit, cont3, i - 1, j - 1, false))) ||
                            (anti && (bridge_of(bit, cont3, i + 1, j - 1, true) || bridge_of(bit, cont3, i - 1, j + 1, true)))) p |= P_LAD;
                        if (j > i && (regs[i] || regs[j])) {
                            n_bridge += (par ? 1 : 0) + (anti ? 1 : 0);
                            if (!wild) n_bkept += ((par && bridge_of(wbit, wcont3, i, j, false)) ? 1 : 0) + ((anti && bridge_of(wbit, wcont3, i, j, true)) ? 1 : 0);
                        }
                    }
                }
            }
            pat[i] = p;
            part[i] = make_short2((short)p0, (short)p1);
        }
        count(wild ? 7 : 6, n_bridge);
        if (!wild) count(8, n_bkept);
        __syncthreads();
        // ---- H, E and B
        auto start = [&](int i, int flag) { return i >= 1 && i < Lab && (pat[i - 1] & flag) && (pat[i] & flag); };
        for (int k = tid; k < Lab; k += 256) {
            bool helix = false;
            for (int i = k - 3; i <= k; ++i) helix = helix || start(i, P_T4);
            const int p = pat[k];
            st[k] = helix ? 1 : ((p & (P_PAR | P_ANTI)) ? ((p & P_LAD) ? 4 : 5) : 0);
        }
        __syncthreads();
        // ---- G: the lanes of this phase write 2 only, and test for 1, 4, 5
        auto heb = [&](int i) { const int v = st[i]; return v == 1 || v == 4 || v == 5; };
        for (int k = tid; k < Lab; k += 256) {
            if (st[k] != 0) continue;
            bool g = false;
            for (int i = k - 2; i <= k; ++i)
                g = g || (start(i, P_T3) && !heb(i) && !heb(i + 1) && !heb(i + 2));             // (TURN_3(i): i + 3 < Lab)
            if (g) st[k] = 2;
        }
        __syncthreads();
        // ---- I: the lanes of this phase write 3 only, and test for 1, 2, 4, 5
        auto hebg = [&](int i) { const int v = st[i]; return v == 1 || v == 2 || v == 4 || v == 5; };
        for (int k = tid; k < Lab; k += 256) {
            if (st[k] != 0) continue;
            bool pi = false;
            for (int i = k - 4; i <= k; ++i)
                pi = pi || (start(i, P_T5) && !hebg(i) && !hebg(i + 1) && !hebg(i + 2) && !hebg(i + 3) && !hebg(i + 4));
            if (pi) st[k] = 3;
        }
        // ---- T, S and the rest: a row's own state and the pattern words only; then the row's share of the counts
        for (int k = tid; k < Lab; k += 256) {
            int state = st[k];
            const int p = pat[k];
            if (state == 0) {
                bool t = false;
#pragma unroll
                for (int n = 3; n <= 5; ++n)
                    for (int i = k - n + 1; i <= k - 1; ++i) t = t || (i >= 0 && (pat[i] & (P_T3 << (n - 3))));
                state = t ? 6 : ((p & P_BEND) ? 7 : 8);
            }
            if (!have[k]) state = 0;
            if (wild) {
                wword[k] = (unsigned)state | (have[k] ? W_PRESENT : 0u) | (cont3(k) ? W_CONT3 : 0u);
                continue;
            }
            const unsigned ww = wword[k];
            const int wstate = (int)(ww & 255u);
            if (regs[k]) {
                if (state) count(8 + state, 1);
                if (have[k] && (ww & W_PRESENT)) {
                    count(17, 1); count(18, state == wstate ? 1 : 0); count(19, class3(state) == class3(wstate) ? 1 : 0);
                }
            }
            count(20, (state == 4 || state == 5) ? 1 : 0);
            count(21, (state >= 1 && state <= 3) ? 1 : 0);
            if (int* rows = rows_p) {
                int* dst = rows + ((long long)b * Lab + k) * 6;
                dst[0] = state; dst[1] = (int)don[k]; dst[2] = acc[k]; dst[3] = (int)part[k].x; dst[4] = (int)part[k].y;
                dst[5] = (regs[k] ? F_REGION : 0) | (have[k] ? F_PRESENT : 0) | (hasH[k] ? F_HAS_H : 0) | ((p & P_PAR) ? F_PARALLEL : 0) |
                         ((p & P_ANTI) ? F_ANTIPARALLEL : 0) | ((p & P_BEND) ? F_BEND : 0) | ((p & (P_T3 | P_T4 | P_T5)) * F_TURN3);
            }
            if (int* classes = classes_p) classes[(long long)b * Lab + k] = state;
        }
        __syncthreads();                                // the wild type's slice is written; every lane has read the staged rows
    };

    pass(true);
    pass(false);
    if (tid == 0) {
        double* out = a.out + (long long)b * a.out_stride;
#pragma unroll
        for (int k = 0; k < ABX_SECONDARY_COLS; ++k) out[k] = (double)cnt[k];
        out[5] = (double)(long long)esum / FIXED;
    }
}

bool unit_pair(const double* p) {
    return std::isfinite(p[0]) && std::isfinite(p[1]) && std::fabs(p[0] * p[0] + p[1] * p[1] - 1.0) <= 1e-9;
}

}  // namespace

extern "C" long long abx_secondary_scores_workspace_bytes(int B, int Lab) {
    if (B <= 0 || Lab <= 0) return 0;
    return (long long)B * slice_words(Lab) * sizeof(unsigned);
}

extern "C" int abx_secondary_scores(const AbxSecondaryArgs* ap, void* workspace, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_secondary_scores: null");
    const AbxSecondaryArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_secondary_scores", 1)) return rc;
    ABX_REQUIRE(a.out && a.chain_id, "abx_secondary_scores: null operand");
    ABX_REQUIRE(a.out_stride >= ABX_SECONDARY_COLS, "abx_secondary_scores: out_stride below ABX_SECONDARY_COLS");
    ABX_REQUIRE(a.Lab <= ABX_SECONDARY_MAX_LAB, "abx_secondary_scores: Lab <= 800 (ABX_SECONDARY_MAX_LAB: the backbone and the bond matrix of a structure are staged in LDS)");
    ABX_REQUIRE(std::isfinite(a.hb_energy) && a.hb_energy < 0.0, "abx_secondary_scores: hb_energy must be finite and below 0");
    ABX_REQUIRE(unit_pair(a.bend), "abx_secondary_scores: bend must be a (cos, sin) pair");
    ABX_REQUIRE(a.pro >= 0 && a.pro <= 20, "abx_secondary_scores: pro must be a residue type 0..20");
    ABX_REQUIRE(workspace != nullptr, "abx_secondary_scores: null workspace");
    if (int rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(secondary_kernel), LDS_MAX, "abx_secondary_scores")) return rc;
    const size_t lds = (size_t)a.Lab * 12 * sizeof(float) + (size_t)a.Lab * words_of(a.Lab) * sizeof(unsigned);
    hipLaunchKernelGGL(secondary_kernel, dim3(a.B), dim3(256), lds, st, a, reinterpret_cast<unsigned*>(workspace));
    return abx_check_launch("abx_secondary_scores");
}
