// Interface analysis of designs (include/abx_hip.h, AbxInterfaceArgs): Shrake-Rupley solvent-accessible surface of the complex and of
// both separated partners in one pass, interface residues and antibody-antigen contacts - the geometric half of upstream's
// InterfaceAnalyzerMover columns (abx/metric.py:28-59, eval/traj_evaluate.py:242-261).  One row of ABX_IFACE_COLS doubles per structure.
//
// Three kernels, no atomics, every float sum in a fixed order, every point test in float64 without fused multiply-add (the operation
// order of the header: the counts are exact integers, equal to those of abx_amd.interface.interface_host):
//   iface_table_kernel   one block per structure: the existing atoms with a positive radius, compacted in slot order (ballot prefix
//                        sums) into a global table - x, y, z, radius as float4 and (slot index << 1 | side) - and one int4 per atom14
//                        slot (acc_alone, acc_cplx, contacts, radius bits; zero radius bits: no atom) for the results.
//   iface_points_kernel  grid (atom tile, structure), 16 waves.  The block copies the structure's table into LDS; every wave owns one
//                        atom at a time (atoms dealt round-robin to the waves of all tiles: the same load everywhere) and runs the
//                        point test of surface_dev.h on it, with the cross-side contact test of a side-A atom.
//   iface_row_kernel     one block per structure: per residue row and per structure, a fixed-order sum; writes the row and `points`.
#include "common.h"
#include "abx_hip.h"
#include "reduce_dev.h"
#include "structure_dev.h"
#include "surface_dev.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int NTB = 1024;              // threads of the point kernel
constexpr int NWB = NTB / 64;          // its waves
constexpr int TILE = 128;              // atoms per workgroup of the point kernel (8 per wave), by which the grid is sized

// bytes of one structure's workspace: header (16), float4 table, int4 per slot, int tag - a multiple of 16
__host__ __device__ constexpr long long ws_stride(int L) { return (16 + 14ll * L * 36 + 15) / 16 * 16; }

using Structure = StructureView<AbxInterfaceArgs>;

struct Workspace {
    int* hdr; float4* tab; int4* slot; int* tag;
    __device__ __forceinline__ Workspace(unsigned char* ws, int b, int L) {
        unsigned char* p = ws + (long long)b * ws_stride(L);
        hdr = reinterpret_cast<int*>(p);
        tab = reinterpret_cast<float4*>(p + 16);
        slot = reinterpret_cast<int4*>(p + 16 + 14ll * L * 16);
        tag = reinterpret_cast<int*>(p + 16 + 14ll * L * 32);
    }
};

__global__ __launch_bounds__(256) void iface_table_kernel(const AbxInterfaceArgs a, unsigned char* __restrict__ ws) {
    __shared__ int wcnt[4];
    const int b = blockIdx.x, tid = threadIdx.x, N14 = a.L * 14;
    const Structure s(a, b);
    const Workspace w(ws, b, a.L);
    int n[1] = {0};                                     // atoms in the chunks already walked
    for (int base = 0; base < N14; base += 256) {
        const int k = base + tid;
        bool ok = false;
        float4 at = make_float4(0.f, 0.f, 0.f, 0.f);
        int tag = 0;
        if (k < N14) {
            ok = table_entry(s, k, a.Lab, at, tag);
            w.slot[k] = make_int4(0, 0, 0, __float_as_int(at.w));
        }
        const unsigned long long bal[1] = {__ballot(ok)};
        int idx[1];
        block_rank<4, 1>(bal, wcnt, idx, n);
        if (ok) {
            w.tab[idx[0]] = at;
            w.tag[idx[0]] = tag;
        }
    }
    if (tid == 0) w.hdr[0] = n[0];
}

__global__ __launch_bounds__(NTB) void iface_points_kernel(const AbxInterfaceArgs a, unsigned char* __restrict__ ws) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, P = a.P;
    const Workspace w(ws, blockIdx.y, a.L);
    const TableLds t(lds, a.L, NTB, w.tab, w.tag, w.hdr[0]);
    const double cut2 = a.cutoff * a.cutoff;
    const int npass = (P + 63) >> 6;
    // every wave owns one atom at a time
    for (int ia = blockIdx.x * NWB + wv; ia < t.n; ia += gridDim.x * NWB) {
        const PointMasks m = point_test<true>(t, ia, a.sphere, P, a.probe, cut2);
        int n_alone = 0, n_cplx = 0;
        for (int k = 0; k < npass; ++k) {
            n_alone += __popcll(__ballot((m.alive >> k) & 1u));
            n_cplx += __popcll(__ballot(((m.alive & ~m.crossed) >> k) & 1u));
        }
        const int ncontact = wave_sum_i(m.contacts);
        if (lane == 0) {
            int4* dst = w.slot + (t.tag[ia] >> 1);
            dst->x = n_alone;
            dst->y = n_cplx;
            dst->z = ncontact;
        }
    }
}

constexpr int NSUM = 12;
__global__ __launch_bounds__(256) void iface_row_kernel(const AbxInterfaceArgs a, const unsigned char* __restrict__ ws) {
    __shared__ double red[4 * NSUM];
    const int b = blockIdx.x, tid = threadIdx.x, L = a.L;
    const Workspace w(const_cast<unsigned char*>(ws), b, L);
    int* pts = a.points ? a.points + (long long)b * L * 28 : nullptr;
    double v[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) v[k] = 0.0;
    for (int row = tid; row < L; row += 256) {
        const bool sideB = row >= a.Lab, reg = a.region && a.region[row];
        bool touched = false;
        for (int sl = 0; sl < 14; ++sl) {
            const int4 c = w.slot[row * 14 + sl];
            const bool ok = c.w != 0;
            if (pts) {
                pts[(row * 14 + sl) * 2] = ok ? c.x : 0;
                pts[(row * 14 + sl) * 2 + 1] = ok ? c.y : 0;
            }
            if (!ok) continue;
            const double R = (double)__int_as_float(c.w) + a.probe, P = (double)a.P;
            const double alone = points_area(R, (double)c.x, P), cplx = points_area(R, (double)c.y, P);
            const double buried = points_area(R, (double)(c.x - c.y), P);
            touched = touched || c.x > c.y;
            v[0] += cplx;
            if (sideB) v[2] += alone;
            else v[1] += alone;
            v[3] += buried;
            if (!sideB) v[4] += buried;
            if (reg) v[5] += buried;
            v[9] += (double)c.z;                        // (contacts are counted on the side-A atom)
            if (reg) v[10] += (double)c.z;
            v[11] += 1.0;
        }
        if (touched) {
            if (sideB) v[7] += 1.0;
            else v[6] += 1.0;
            if (reg) v[8] += 1.0;
        }
    }
    block_sum_d<NSUM>(v, red);
    if (tid < NSUM) {
        double r = v[0];
#pragma unroll
        for (int k = 1; k < NSUM; ++k) r = tid == k ? v[k] : r;
        a.out[(long long)b * a.out_stride + tid] = r;
    }
}

}  // namespace

extern "C" long long abx_interface_scores_workspace_bytes(int B, int L, int P) {
    if (B <= 0 || L <= 0 || P <= 0) return 0;
    return (long long)B * ws_stride(L);
}

extern "C" int abx_interface_scores(const AbxInterfaceArgs* ap, void* workspace, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_interface_scores: null");
    const AbxInterfaceArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_interface_scores", 1)) return rc;
    ABX_REQUIRE(a.sphere && a.out, "abx_interface_scores: null operand");
    ABX_REQUIRE(a.P >= 1 && a.P <= 1024, "abx_interface_scores: P must be in 1..1024");
    ABX_REQUIRE(a.out_stride >= ABX_IFACE_COLS, "abx_interface_scores: out_stride below ABX_IFACE_COLS");
    ABX_REQUIRE(std::isfinite(a.probe) && a.probe >= 0.0, "abx_interface_scores: probe must be >= 0");
    ABX_REQUIRE(std::isfinite(a.cutoff) && a.cutoff > 0.0, "abx_interface_scores: cutoff must be > 0");
    ABX_REQUIRE(table_lds_bytes(a.L, NWB) <= ABX_LDS_LIMIT, "abx_interface_scores: the atom table does not fit the LDS of a CU (L <= 541)");
    ABX_REQUIRE(workspace != nullptr, "abx_interface_scores: null workspace");
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    hipLaunchKernelGGL(iface_table_kernel, dim3(a.B), dim3(256), 0, st, a, ws);
    int rc = abx_check_launch("abx_interface_scores(atom table)");
    if (rc) return rc;
    rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(iface_points_kernel), ABX_LDS_LIMIT, "abx_interface_scores");
    if (rc) return rc;
    const int tiles = (a.L * 14 + TILE - 1) / TILE;
    hipLaunchKernelGGL(iface_points_kernel, dim3(tiles, a.B), dim3(NTB), (int)table_lds_bytes(a.L, NWB), st, a, ws);
    rc = abx_check_launch("abx_interface_scores(points)");
    if (rc) return rc;
    hipLaunchKernelGGL(iface_row_kernel, dim3(a.B), dim3(256), 0, st, a, ws);
    return abx_check_launch("abx_interface_scores");
}
