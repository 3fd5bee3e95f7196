// Polar interface contacts of designs (include/abx_hip.h, AbxPolarArgs): heavy-atom hydrogen bonds, salt bridges and the polar atoms that
// binding buries without a partner - the chemical columns upstream takes from InterfaceAnalyzerMover beside dG and dSASA (hbonds_int,
// delta_unsatHbonds; abx/metric.py:28-59, eval/traj_evaluate.py:233-261).  One row of ABX_POLAR_COLS doubles per structure.
//
// One kernel, one workgroup of 16 waves per structure, no global atomics, every test in float64 without fused multiply-add (the
// operation order of the header: the counts are exact integers, equal to those of abx_amd.polar.polar_host):
//   0. one byte per atom14 slot (it exists) and per row (its residue type), in LDS that later holds the counters.
//   1. the polar atoms (a role bit in `table`, slot and antecedent slot exist) are compacted in slot order by ballot prefix sums into
//      LDS: x, y, z, flags | antecedent x, y, z, point counts; at most 5 per residue (Arg: N, O, NE, NH1, NH2).
//   2. wave w owns the atoms w, w + 16, ...; its lanes take the partners i + 1 + lane, + 64, ...: every unordered pair once.  A bond adds
//      to the two atoms' (same-side, cross-side) counters and to the row's counters by integer LDS atomics (integers commute).  A salt
//      bridge is counted by the FIRST atom pair of its residue pair that qualifies (the atoms of a row are neighbours in the table).
//   3. the burial columns from the point counts of the table entries.  The two areas over all atom14 slots are summed before the pair
//      loop: per thread in slot order, wave shuffles, then the 16 partials in wave order.
#include "common.h"
#include "abx_hip.h"
#include "reduce_dev.h"
#include "structure_dev.h"
#include "surface_dev.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 1024;               // threads of the workgroup
constexpr int NW = NT / 64;            // its waves
constexpr int PER_RES = 5;             // table entries per residue row the LDS is sized for
constexpr int NCNT = 16;               // integer counters (the columns 0-9 and 12)

// flags of a table entry (float4.w of the atom): the role bits of `table`, then
constexpr int F_BB = 1 << 4, F_REGION = 1 << 5, F_SIDEB = 1 << 6;      // bits 8-11: slot, bits 12-: row

// two float4 and two counters per entry, four counters per row, the counters and the area partials
__host__ __device__ constexpr long long polar_lds_bytes(int L) { return (40ll * PER_RES + 16) * L + 512; }

using Structure = StructureView<AbxPolarArgs>;

__device__ __forceinline__ bool salt_roles(int fa, int fb) {
    return ((fa & ABX_POLAR_CATION) && (fb & ABX_POLAR_ANION)) || ((fa & ABX_POLAR_ANION) && (fb & ABX_POLAR_CATION));
}

__device__ __forceinline__ double dist2(const float4& a, const float4& b) {
    const double dx = (double)b.x - (double)a.x, dy = (double)b.y - (double)a.y, dz = (double)b.z - (double)a.z;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(NT) void polar_kernel(const AbxPolarArgs a, double cos2) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int L = a.L, N14 = L * 14, cap = PER_RES * L;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float4* A = reinterpret_cast<float4*>(lds);                               // [cap] x, y, z, flags
    float4* U = A + cap;                                                      // [cap] antecedent x, y, z, acc_alone << 16 | acc_cplx
    int* bond = reinterpret_cast<int*>(U + cap);                              // [cap][2] same-side, cross-side bonds of the entry
    int* rowc = bond + 2 * cap;                                               // [L][4] cross-side, same-side bonds, salt partners, unsatisfied
    int* cnt = rowc + 4 * L;                                                  // [NCNT]
    int* wcnt = cnt + NCNT;                                                   // [NW]
    double* part = reinterpret_cast<double*>(lds + polar_lds_bytes(L) - 256); // [NW][2] area partials
    const int* pts = a.points ? a.points + (long long)b * N14 * 2 : nullptr;
    unsigned char* ex = reinterpret_cast<unsigned char*>(bond);               // [N14] the slot exists; [L] residue types (until the counters are zeroed)
    unsigned char* aab = ex + N14;

    // ---- 0. which slots exist, and the residue types (a pass of its own: every pass keeps few pointers live)
    {
        const Structure s(a, b);
        for (int k = tid; k < N14; k += NT) {
            const int row = k / 14, sl = k - row * 14, aa = s.aatype(row);
            ex[k] = s.exists(row, sl, aa) ? 1 : 0;
            if (sl == 0) aab[row] = (unsigned char)aa;
        }
    }
    __syncthreads();
    // ---- 1. the table, in slot order
    const float* pred = a.pred_atom14 + (long long)b * a.pred_sb;
    int found[1] = {0};
    for (int base = 0; base < N14; base += NT) {
        const int k = base + tid;
        bool ok = false;
        float4 at = make_float4(0.f, 0.f, 0.f, 0.f), an = at;
        if (k < N14) {
            const int row = k / 14, sl = k - row * 14;
            const int t = a.table[aab[row] * 14 + sl], as = (t >> 8) & 15;
            ok = (t & (ABX_POLAR_DONOR | ABX_POLAR_ACCEPTOR)) != 0 && as < 14 && ex[k] && ex[row * 14 + as];
            if (ok) {
                const float* x = (row < a.Lpred ? pred : a.gt_atom14) + (long long)row * 42;
                const int fl = (t & 15) | (sl < 4 ? F_BB : 0) | (row >= a.Lab ? F_SIDEB : 0) | (sl << 8) | (row << 12);
                at = make_float4(x[3 * sl], x[3 * sl + 1], x[3 * sl + 2], __int_as_float(fl));
                an = make_float4(x[3 * as], x[3 * as + 1], x[3 * as + 2], 0.f);
            }
        }
        const unsigned long long bal[1] = {__ballot(ok)};
        int rank[1];
        block_rank<NW, 1>(bal, wcnt, rank, found);
        const int idx = rank[0];
        if (ok && idx < cap) {                          // (a table with more than PER_RES polar atoms per residue is cut, never overrun)
            A[idx] = at;
            U[idx] = an;
        }
    }
    const int n = found[0] < cap ? found[0] : cap;
    __syncthreads();
    // the region bit and the point counts of the entries
    for (int i = tid; i < n; i += NT) {
        const int fl = __float_as_int(A[i].w), row = fl >> 12, k = row * 14 + ((fl >> 8) & 15);
        if (a.region && a.region[row]) A[i].w = __int_as_float(fl | F_REGION);
        if (pts) U[i].w = __int_as_float(((pts[2 * k] & 0xffff) << 16) | (pts[2 * k + 1] & 0xffff));
    }
    // the buried area of all atoms, split by element: per thread in slot order, wave shuffles; the partials are summed in wave order
    // at the end
    if (pts) {
        double pol = 0.0, apol = 0.0;
        for (int k = tid; k < N14; k += NT) {
            const int row = k / 14, sl = k - row * 14, aa = aab[row];
            const float r = a.radius[aa * 14 + sl];
            if (!(r > 0.f && ex[k])) continue;
            const double R = (double)r + a.probe;
            const double area = points_area(R, (double)(pts[2 * k] - pts[2 * k + 1]), (double)a.P);
            if (a.table[aa * 14 + sl] & ABX_POLAR_ELEMENT) pol += area;
            else apol += area;
        }
        pol = wave_sum_d(pol);
        apol = wave_sum_d(apol);
        if (lane == 0) {
            part[2 * wv] = pol;
            part[2 * wv + 1] = apol;
        }
    }
    int* bonds_out = a.bonds ? a.bonds + (long long)b * N14 * 2 : nullptr;
    if (bonds_out)
        for (int k = tid; k < 2 * N14; k += NT) bonds_out[k] = 0;
    __syncthreads();                                    // ex and aab have been read: their bytes become counters
    for (int i = tid; i < 2 * cap + 4 * L + NCNT; i += NT) bond[i] = 0;       // bond, rowc and cnt are contiguous
    __syncthreads();

    // ---- 2. the pairs
    const double min2 = a.hb_min * a.hb_min, max2 = a.hb_max * a.hb_max, salt2 = a.salt * a.salt;
    for (int i = wv; i < n; i += NW) {
        const float4 pa = A[i], ua = U[i];
        const int fa = __float_as_int(pa.w), rowa = fa >> 12;
        for (int j = i + 1 + lane; j < n; j += 64) {
            const float4 pb = A[j];
            const int fb = __float_as_int(pb.w), rowb = fb >> 12;
            if (rowb == rowa) continue;
            const double dx = (double)pb.x - (double)pa.x, dy = (double)pb.y - (double)pa.y, dz = (double)pb.z - (double)pa.z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            const bool cross = ((fa ^ fb) & F_SIDEB) != 0, reg = ((fa | fb) & F_REGION) != 0;
            if (cross && d2 <= salt2 && salt_roles(fa, fb)) {
                // the first qualifying atom pair (i', j') of this residue pair in table order counts it
                int i0 = i, j0 = j;
                while (i0 > 0 && (__float_as_int(A[i0 - 1].w) >> 12) == rowa) --i0;
                while (j0 > 0 && (__float_as_int(A[j0 - 1].w) >> 12) == rowb) --j0;
                bool first = true;
                for (int ii = i0; ii <= i && first; ++ii) {
                    const float4 qa = A[ii];
                    for (int jj = j0; jj < n && (ii < i || jj < j); ++jj) {
                        const float4 qb = A[jj];
                        if ((__float_as_int(qb.w) >> 12) != rowb) break;
                        if (salt_roles(__float_as_int(qa.w), __float_as_int(qb.w)) && dist2(qa, qb) <= salt2) { first = false; break; }
                    }
                }
                if (first) {
                    atomicAdd(&cnt[4], 1);
                    if (reg) atomicAdd(&cnt[5], 1);
                    atomicAdd(&rowc[4 * rowa + 2], 1);
                    atomicAdd(&rowc[4 * rowb + 2], 1);
                }
            }
            const bool roles = ((fa & ABX_POLAR_DONOR) && (fb & ABX_POLAR_ACCEPTOR)) || ((fa & ABX_POLAR_ACCEPTOR) && (fb & ABX_POLAR_DONOR));
            if (!roles || !(d2 >= min2 && d2 <= max2)) continue;
            const double ux = (double)ua.x - (double)pa.x, uy = (double)ua.y - (double)pa.y, uz = (double)ua.z - (double)pa.z;
            const double ta = (ux * dx + uy * dy) + uz * dz, uu = (ux * ux + uy * uy) + uz * uz;
            if (!(ta <= 0.0 && ta * ta >= cos2 * (uu * d2))) continue;
            const float4 ub = U[j];
            const double vx = (double)ub.x - (double)pb.x, vy = (double)ub.y - (double)pb.y, vz = (double)ub.z - (double)pb.z;
            const double tb = (vx * dx + vy * dy) + vz * dz, vv = (vx * vx + vy * vy) + vz * vz;
            if (!(tb >= 0.0 && tb * tb >= cos2 * (vv * d2))) continue;
            atomicAdd(&cnt[12], 1);
            atomicAdd(&bond[2 * i + (cross ? 1 : 0)], 1);
            atomicAdd(&bond[2 * j + (cross ? 1 : 0)], 1);
            if (cross) {
                atomicAdd(&cnt[0], 1);
                if (fa & fb & F_BB) atomicAdd(&cnt[1], 1);
                if (reg) atomicAdd(&cnt[2], 1);
            } else if (reg) {
                atomicAdd(&cnt[3], 1);
            }
        }
    }
    __syncthreads();

    // ---- 3. burial of the polar atoms
    if (pts) {
        for (int base = 0; base < n; base += NT) {
            const int i = base + tid;
            bool at_int = false, buried = false, unsat = false, ureg = false;
            if (i < n) {
                const int fl = __float_as_int(A[i].w), pc = __float_as_int(U[i].w), alone = pc >> 16, cplx = pc & 0xffff;
                at_int = alone > cplx;
                buried = alone > 0 && cplx == 0;
                unsat = buried && bond[2 * i] + bond[2 * i + 1] == 0;
                ureg = unsat && (fl & F_REGION);
                if (unsat) atomicAdd(&rowc[4 * (fl >> 12) + 3], 1);
            }
            const int c6 = __popcll(__ballot(at_int)), c7 = __popcll(__ballot(buried)), c8 = __popcll(__ballot(unsat)), c9 = __popcll(__ballot(ureg));
            if (lane == 0) {
                atomicAdd(&cnt[6], c6);
                atomicAdd(&cnt[7], c7);
                atomicAdd(&cnt[8], c8);
                atomicAdd(&cnt[9], c9);
            }
        }
    }
    for (int i = tid; i < n; i += NT) {
        const int row = __float_as_int(A[i].w) >> 12;
        if (bond[2 * i + 1]) atomicAdd(&rowc[4 * row], bond[2 * i + 1]);
        if (bond[2 * i]) atomicAdd(&rowc[4 * row + 1], bond[2 * i]);
    }
    __syncthreads();                                    // counters, partials and the zeros of `bonds` are complete
    if (bonds_out)
        for (int i = tid; i < n; i += NT) {
            const int fl = __float_as_int(A[i].w), k = (fl >> 12) * 14 + ((fl >> 8) & 15);
            bonds_out[2 * k] = bond[2 * i];
            bonds_out[2 * k + 1] = bond[2 * i + 1];
        }
    if (a.rows)
        for (int k = tid; k < 4 * L; k += NT) a.rows[(long long)b * 4 * L + k] = ((k & 3) == 3 && !pts) ? -1 : rowc[k];
    if (tid < ABX_POLAR_COLS) {
        double v;
        if (tid == 13) v = (double)n;
        else if (tid == 10 || tid == 11) {
            v = -1.0;
            if (pts) {
                v = 0.0;
                for (int w = 0; w < NW; ++w) v += part[2 * w + (tid - 10)];
            }
        } else if (tid >= 6 && tid <= 9 && !pts) v = -1.0;
        else v = (double)cnt[tid];
        a.out[(long long)b * a.out_stride + tid] = v;
    }
}

}  // namespace

extern "C" long long abx_polar_scores_workspace_bytes(int B, int L) {
    (void)B; (void)L;
    return 0;
}

extern "C" long long abx_polar_scores_lds_bytes(int L) { return L > 0 ? polar_lds_bytes(L) : 0; }

extern "C" int abx_polar_scores(const AbxPolarArgs* ap, void* workspace, hipStream_t st) {
    (void)workspace;
    ABX_REQUIRE(ap != nullptr, "abx_polar_scores: null");
    const AbxPolarArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_polar_scores", 1)) return rc;
    ABX_REQUIRE(a.table && a.out, "abx_polar_scores: null operand");
    ABX_REQUIRE(a.out_stride >= ABX_POLAR_COLS, "abx_polar_scores: out_stride below ABX_POLAR_COLS");
    ABX_REQUIRE(std::isfinite(a.hb_min) && std::isfinite(a.hb_max) && a.hb_min >= 0.0 && a.hb_min <= a.hb_max,
                "abx_polar_scores: needs 0 <= hb_min <= hb_max");
    ABX_REQUIRE(std::isfinite(a.hb_angle) && a.hb_angle >= 90.0 && a.hb_angle < 180.0, "abx_polar_scores: hb_angle must be in [90, 180) degrees");
    const double c = std::cos(a.hb_angle * (3.14159265358979323846 / 180.0));
    const double cos2 = a.hb_angle == 90.0 ? 0.0 : a.hb_cos2;
    ABX_REQUIRE(std::isfinite(a.hb_cos2) && a.hb_cos2 >= 0.0 && a.hb_cos2 < 1.0 && std::fabs(a.hb_cos2 - c * c) <= 1e-12,
                "abx_polar_scores: hb_cos2 is not cos^2(hb_angle)");
    ABX_REQUIRE(std::isfinite(a.salt) && a.salt >= 0.0, "abx_polar_scores: salt must be >= 0");
    if (a.points) {
        ABX_REQUIRE(a.P >= 1 && a.P <= 1024, "abx_polar_scores: P must be in 1..1024");
        ABX_REQUIRE(std::isfinite(a.probe) && a.probe >= 0.0, "abx_polar_scores: probe must be >= 0");
    }
    ABX_REQUIRE(polar_lds_bytes(a.L) <= ABX_LDS_LIMIT, "abx_polar_scores: the polar-atom table does not fit the LDS of a CU (L <= 756)");
    int rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(polar_kernel), ABX_LDS_LIMIT, "abx_polar_scores");
    if (rc) return rc;
    hipLaunchKernelGGL(polar_kernel, dim3(a.B), dim3(NT), (int)polar_lds_bytes(a.L), st, a, cos2);
    return abx_check_launch("abx_polar_scores");
}
