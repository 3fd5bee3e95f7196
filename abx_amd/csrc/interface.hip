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
//                        atom at a time (atoms dealt round-robin to the waves of all tiles: the same load everywhere).  It scans the
//                        table 64 atoms per step - float64 distance, the conservative sphere-sphere test d < R_a + R_b + 1e-3 and, for
//                        a side-A atom, the cross-side contact test - and appends the neighbours by ballot to the wave's LDS list.
//                        Then its lanes take the points lane, lane + 64, ... and walk the list: an own-side occluder ends the point
//                        (it is lost to every surface), an other-side occluder is only recorded.  The state of a lane's <= 16 points
//                        is two bit masks, so a list that fills up (192 entries) is worked off and reused: no bound on the neighbours.
//   iface_row_kernel     one block per structure: per residue row and per structure, a fixed-order sum; writes the row and `points`.
//
// Rounding cannot make the prefilter drop an occluder: a point lies within 1e-12 of R_a from its centre, so an occluding atom has
// d <= R_a + R_b + 1e-12, six orders inside the slack.
#include "common.h"
#include "abx_hip.h"
#include "reduce_dev.h"
#include "structure_dev.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int NTB = 1024;              // threads of the point kernel
constexpr int NWB = NTB / 64;          // its waves
constexpr int CAP = 192;               // neighbour list entries per wave (worked off when fewer than 64 are free)
constexpr int TILE = 128;              // atoms per workgroup of the point kernel (8 per wave), by which the grid is sized
constexpr double SLACK = 1e-3;         // Angstrom added to R_a + R_b in the neighbour prefilter
constexpr double FOUR_PI = 12.566370614359172;

__host__ __device__ constexpr long long points_lds_bytes(int L) { return 14ll * L * 20 + NWB * CAP * 4; }
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
    int before = 0;                                     // atoms in the chunks already walked
    for (int base = 0; base < N14; base += 256) {
        const int k = base + tid;
        bool ok = false;
        float4 at = make_float4(0.f, 0.f, 0.f, 0.f);
        int row = 0;
        if (k < N14) {
            row = k / 14;
            const int sl = k - row * 14, aa = s.aatype(row);
            const float r = s.radius[aa * 14 + sl];
            ok = r > 0.f && s.exists(row, sl, aa);
            if (ok) {
                const float* x = s.xyz(row, sl);
                at = make_float4(x[0], x[1], x[2], r);
            }
            w.slot[k] = make_int4(0, 0, 0, ok ? __float_as_int(r) : 0);
        }
        const unsigned long long bal = __ballot(ok);
        __syncthreads();                                // the previous chunk's counts have been read
        if ((tid & 63) == 0) wcnt[tid >> 6] = __popcll(bal);
        __syncthreads();
        int idx = before + lanes_below(bal);
        for (int v = 0; v < (tid >> 6); ++v) idx += wcnt[v];
        before += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (ok) {
            w.tab[idx] = at;
            w.tag[idx] = (k << 1) | (row >= a.Lab ? 1 : 0);
        }
    }
    if (tid == 0) w.hdr[0] = before;
}

__global__ __launch_bounds__(NTB) void iface_points_kernel(const AbxInterfaceArgs a, unsigned char* __restrict__ ws) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int N14 = a.L * 14, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y, P = a.P;
    float4* tab = reinterpret_cast<float4*>(lds);                       // [n] x, y, z, radius
    int* tag = reinterpret_cast<int*>(lds + 16ll * N14);                // [n] slot index << 1 | side
    int* list = reinterpret_cast<int*>(lds + 20ll * N14) + wv * CAP;    // this wave's neighbours: table index | other side << 31
    const Workspace w(ws, b, a.L);
    const int n = w.hdr[0];
    for (int i = tid; i < n; i += NTB) {
        tab[i] = w.tab[i];
        tag[i] = w.tag[i];
    }
    __syncthreads();
    const double probe = a.probe, cut2 = a.cutoff * a.cutoff;
    const int npass = (P + 63) >> 6;
    for (int ia = blockIdx.x * NWB + wv; ia < n; ia += gridDim.x * NWB) {
        const float4 me = tab[ia];
        const int mtag = tag[ia], mside = mtag & 1;
        const double xa = (double)me.x, ya = (double)me.y, za = (double)me.z, Ra = (double)me.w + probe;
        // bit k of a mask: this lane's point k * 64 + lane.  alive: occluded by no own-side atom so far; crossed: by an other-side one
        unsigned alive = 0, crossed = 0;
        for (int k = 0; k < npass; ++k) alive |= (k * 64 + lane < P ? 1u : 0u) << k;
        int cnt = 0, ncontact = 0;

        // the points of this atom against the cnt neighbours of the list
        auto work_off = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");     // the list entries of the other lanes (one wave: in order)
            __builtin_amdgcn_wave_barrier();
            for (int k = 0; k < npass; ++k) {
                bool live = (alive >> k) & 1u;
                if (__ballot(live) == 0ull) continue;
                const int p = min(k * 64 + lane, P - 1);
                const double px = xa + Ra * a.sphere[3 * p], py = ya + Ra * a.sphere[3 * p + 1], pz = za + Ra * a.sphere[3 * p + 2];
                bool cross = false;
                for (int j = 0; j < cnt; ++j) {
                    const int e = list[j];
                    const float4 o = tab[e & 0x7fffffff];
                    const double dx = px - (double)o.x, dy = py - (double)o.y, dz = pz - (double)o.z;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    const double Rb = (double)o.w + probe;
                    if (live && d2 < Rb * Rb) {
                        if (e < 0) cross = true;
                        else live = false;
                    }
                    if (__ballot(live) == 0ull) break;
                }
                if (!live) alive &= ~(1u << k);
                if (cross) crossed |= 1u << k;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");     // the list is free again
        };

        bool dead = false;                              // no point is left: only the contacts still need the scan
        for (int base = 0; base < n; base += 64) {
            if (dead && mside != 0) break;
            const int j = base + lane;
            bool nb = false, other = false;
            if (j < n && j != ia) {
                const float4 o = tab[j];
                other = (tag[j] & 1) != mside;
                const double dx = xa - (double)o.x, dy = ya - (double)o.y, dz = za - (double)o.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                const double rs = (Ra + ((double)o.w + probe)) + SLACK;
                nb = !dead && d2 < rs * rs;
                if (other && mside == 0 && d2 < cut2) ++ncontact;
            }
            const unsigned long long bal = __ballot(nb);
            if (nb) list[cnt + lanes_below(bal)] = j | (other ? (int)0x80000000 : 0);
            cnt += __popcll(bal);
            if (cnt > CAP - 64) {
                work_off();
                cnt = 0;
                dead = __ballot(alive != 0u) == 0ull;
            }
        }
        if (cnt > 0) work_off();
        int n_alone = 0, n_cplx = 0;
        for (int k = 0; k < npass; ++k) {
            n_alone += __popcll(__ballot((alive >> k) & 1u));
            n_cplx += __popcll(__ballot(((alive & ~crossed) >> k) & 1u));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ncontact += __shfl_xor(ncontact, o, 64);
        if (lane == 0) {
            int4* dst = w.slot + (mtag >> 1);
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
            const double R = (double)__int_as_float(c.w) + a.probe;
            const double sphere = FOUR_PI * (R * R);
            const double alone = sphere * (double)c.x / (double)a.P, cplx = sphere * (double)c.y / (double)a.P;
            const double buried = sphere * (double)(c.x - c.y) / (double)a.P;
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
    ABX_REQUIRE(points_lds_bytes(a.L) <= ABX_LDS_LIMIT, "abx_interface_scores: the atom table does not fit the LDS of a CU (L <= 541)");
    ABX_REQUIRE(workspace != nullptr, "abx_interface_scores: null workspace");
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    hipLaunchKernelGGL(iface_table_kernel, dim3(a.B), dim3(256), 0, st, a, ws);
    int rc = abx_check_launch("abx_interface_scores(atom table)");
    if (rc) return rc;
    rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(iface_points_kernel), ABX_LDS_LIMIT, "abx_interface_scores");
    if (rc) return rc;
    const int tiles = (a.L * 14 + TILE - 1) / TILE;
    hipLaunchKernelGGL(iface_points_kernel, dim3(tiles, a.B), dim3(NTB), (int)points_lds_bytes(a.L), st, a, ws);
    rc = abx_check_launch("abx_interface_scores(points)");
    if (rc) return rc;
    hipLaunchKernelGGL(iface_row_kernel, dim3(a.B), dim3(256), 0, st, a, ws);
    return abx_check_launch("abx_interface_scores");
}
