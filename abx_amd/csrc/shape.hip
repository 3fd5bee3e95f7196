// Shape complementarity of the interface (include/abx_hip.h, AbxShapeArgs): the Sc statistic of Lawrence & Colman (1993) on the contact
// part of the molecular surface of both separated partners.  One row of ABX_SHAPE_COLS doubles per structure.  Every decision - which
// dot is buried, which is trimmed, which is the nearest - is taken in float64 without fused multiply-add in the operation order of the
// header, so the counts equal those of abx_amd.shape.shape_host and the medians differ by the few ulp of exp and sqrt only.
//
// `points` of abx_interface_scores for the same structures names the atoms to process (acc_alone > acc_cplx) and fixes every list size
// and every atom's offset before a dot is generated: the lists are compacted without atomics and in (row, slot, point) order.
// Five kernels, no global atomics, a structure's row depends on its own inputs only:
//   shape_offsets_kernel  one workgroup per structure: the atom table of the interface kernel (x, y, z, radius; slot index << 1 | side),
//                         the interface atoms with the offsets of their buried and open dots (prefix sums in atom order), the list
//                         sizes; a structure whose sizes exceed max_dots, or whose `points` cannot be, is marked and skipped from here on.
//   shape_dots_kernel     one wave per interface atom, the structure's atom table in LDS: the point test of surface_dev.h, the one that
//                         iface_points_kernel runs, then the buried dots go to the I list and the open ones to the E list of the atom's side
//                         by ballot prefix sums over the points in ascending order.  A wave never writes past the segment that
//                         `points` promised; an atom whose counts disagree marks the structure.
//   shape_trim_kernel     one workgroup per (side, structure): a buried dot with an open dot of its side within `trim` goes; the E list
//                         through LDS in chunks, every lane reads the same entry (a broadcast); the kept dots are compacted in place.
//   shape_match_kernel    grid (at most 8 workgroups, side, structure), each walking tiles of 256 kept dots: one thread per dot, the other
//                         side's kept dots through LDS in chunks of j_chunk; nearest dot, ties to the lowest index; S and d2 to the
//                         workspace.  A workgroup beyond the count leaves before any barrier, an empty list is never read.  (A grid
//                         sized by max_dots spends 0.4 ms dispatching 6 400 workgroups of which 600 have a tile.)
//   shape_reduce_kernel   one workgroup per structure: the medians by an eight-pass radix select on the order-preserving integer image
//                         of the doubles (a 256-bin LDS histogram per pass), and the row.
#include "common.h"
#include "abx_hip.h"
#include "reduce_dev.h"
#include "structure_dev.h"
#include "surface_dev.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                // threads of the offsets, match and reduce kernels
constexpr int NW = NT / 64;
constexpr int NTD = 1024;              // threads of the dot kernel
constexpr int NWD = NTD / 64;
constexpr int DOT_BLOCKS = 4;          // workgroups of the dot kernel per structure (64 waves for a few hundred interface atoms)
constexpr int NTT = 1024;              // threads of the trim kernel = open dots per LDS chunk
constexpr int NWT = NTT / 64;
constexpr int J_CHUNK = 1024;          // default and largest chunk of the other side's dots in the match kernel
constexpr int MATCH_TILES = 8;         // most workgroups of the match kernel per (side, structure): each walks the tiles tile, tile + 8, ...
constexpr int MAX_DOTS = 1 << 20;

struct Dot { double x, y, z; int info, pad; };      // a buried dot: position, row << 10 | point
struct Open { double x, y, z; };                    // an open dot: position

// bytes of one structure's workspace: header (64), float4 table, int4 per interface atom, int tag, then per side and dot of capacity:
// I (32), E (24), S (8), d2 (8) - a multiple of 16
__host__ __device__ constexpr long long ws_stride(int L, int M) { return (64 + 14ll * L * 36 + 144ll * M + 15) / 16 * 16; }

using Structure = StructureView<AbxShapeArgs>;

// header words
enum { H_NTAB = 0, H_NATOM = 1, H_NI = 2, H_NE = 4, H_NT = 6, H_BAD = 8, H_MISMATCH = 9 };

struct Workspace {
    int* hdr; float4* tab; int4* atoms; int* tag; Dot* I; Open* E; double* S; double* D2;
    int M;
    __device__ __forceinline__ Workspace(unsigned char* ws, int b, int L, int M_) : M(M_) {
        unsigned char* p = ws + (long long)b * ws_stride(L, M_);
        hdr = reinterpret_cast<int*>(p);
        tab = reinterpret_cast<float4*>(p + 64);
        atoms = reinterpret_cast<int4*>(p + 64 + 14ll * L * 16);
        tag = reinterpret_cast<int*>(p + 64 + 14ll * L * 32);
        unsigned char* d = p + 64 + 14ll * L * 36;
        I = reinterpret_cast<Dot*>(d);
        E = reinterpret_cast<Open*>(d + 64ll * M_);
        S = reinterpret_cast<double*>(d + 112ll * M_);
        D2 = reinterpret_cast<double*>(d + 128ll * M_);
    }
    __device__ __forceinline__ bool skipped() const { return hdr[H_BAD] != 0 || hdr[H_MISMATCH] != 0; }
};

__global__ __launch_bounds__(NT) void shape_offsets_kernel(const AbxShapeArgs a, unsigned char* __restrict__ ws) {
    __shared__ int wtot[NW * 6];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, N14 = a.L * 14;
    const Structure s(a, b);
    const Workspace w(ws, b, a.L, a.max_dots);
    const int* pts = a.points + (long long)b * a.L * 28;
    // so far: dots I of side A, E of A, I of B, E of B, then atoms and interface atoms
    int run[6] = {0, 0, 0, 0, 0, 0};
    bool bad = false;
    for (int base = 0; base < N14; base += NT) {
        const int k = base + tid;
        bool ok = false, sel = false;
        float4 at = make_float4(0.f, 0.f, 0.f, 0.f);
        int tag = 0, nb = 0, ne = 0;
        if (k < N14) {
            ok = table_entry(s, k, a.Lab, at, tag);
            const int alone = pts[2 * k], cplx = pts[2 * k + 1];
            if (alone < 0 || cplx < 0 || alone > a.P || cplx > alone) bad = true;
            else if (alone > cplx) {
                if (ok) {
                    sel = true;
                    nb = alone - cplx;
                    ne = cplx;
                } else bad = true;                          // buried dots of an atom that is not there
            }
        }
        const bool sideB = tag & 1;
        const unsigned long long bo = __ballot(ok), bs = __ballot(sel);
        const int v[4] = {sideB ? 0 : nb, sideB ? 0 : ne, sideB ? nb : 0, sideB ? ne : 0};
        int col[6], off[6];                                 // inclusive scans (lane 63: the wave's totals), exclusive places
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            col[q] = wave_scan_i(v[q], lane);
            off[q] = col[q] - v[q];
        }
        col[4] = __popcll(bo); off[4] = lanes_below(bo);
        col[5] = __popcll(bs); off[5] = lanes_below(bs);
        block_offsets<NW, 6>(col, wtot, off, run);
        const int idx = off[4], ia = off[5];
        if (ok) {
            w.tab[idx] = at;
            w.tag[idx] = tag;
        }
        if (sel) w.atoms[ia] = make_int4(idx, sideB ? off[2] : off[0], sideB ? off[3] : off[1], (nb << 16) | ne);   // ia < N14
    }
    const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
    if (tid == 0) {
        w.hdr[H_NTAB] = run[4];
        w.hdr[H_NATOM] = run[5];
        w.hdr[H_NI] = run[0]; w.hdr[H_NI + 1] = run[2];
        w.hdr[H_NE] = run[1]; w.hdr[H_NE + 1] = run[3];
        w.hdr[H_NT] = 0; w.hdr[H_NT + 1] = 0;
        const int M = a.max_dots;
        w.hdr[H_BAD] = (any_bad || run[0] > M || run[1] > M || run[2] > M || run[3] > M) ? 1 : 0;
        w.hdr[H_MISMATCH] = 0;
    }
}

__global__ __launch_bounds__(NTD) void shape_dots_kernel(const AbxShapeArgs a, unsigned char* __restrict__ ws) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, P = a.P;
    const Workspace w(ws, blockIdx.y, a.L, a.max_dots);
    if (w.hdr[H_BAD]) return;
    const int natom = w.hdr[H_NATOM];
    if ((int)blockIdx.x * NWD >= natom) return;         // the whole workgroup: no barrier has been passed
    const TableLds t(lds, a.L, NTD, w.tab, w.tag, w.hdr[H_NTAB]);
    const int npass = (P + 63) >> 6;
    for (int q = blockIdx.x * NWD + wv; q < natom; q += gridDim.x * NWD) {
        const int4 ent = w.atoms[q];
        const int ia = ent.x;
        // the masks that iface_points_kernel counted into `points`: the same function
        const PointMasks m = point_test<false>(t, ia, a.sphere, P, a.probe, 0.0);
        const float4 me = t.tab[ia];
        const int mtag = t.tag[ia], mside = mtag & 1;
        const double xa = (double)me.x, ya = (double)me.y, za = (double)me.z, ra = (double)me.w;
        // the dots, points ascending: buried ones to the I segment, open ones to the E segment that `points` promised
        const int want_b = ent.w >> 16, want_e = ent.w & 0xffff, row = (mtag >> 1) / 14;
        Dot* I = w.I + (long long)mside * w.M + ent.y;
        Open* E = w.E + (long long)mside * w.M + ent.z;
        int nb = 0, ne = 0;
        for (int k = 0; k < npass; ++k) {
            const bool live = (m.alive >> k) & 1u, cr = (m.crossed >> k) & 1u;
            const bool bur = live && cr, op = live && !cr;
            const unsigned long long bb = __ballot(bur), be = __ballot(op);
            const int p = min(k * 64 + lane, P - 1);
            const double mx = xa + ra * a.sphere[3 * p], my = ya + ra * a.sphere[3 * p + 1], mz = za + ra * a.sphere[3 * p + 2];
            const int ib = nb + lanes_below(bb), ie = ne + lanes_below(be);
            if (bur && ib < want_b) {
                Dot d;
                d.x = mx; d.y = my; d.z = mz; d.info = (row << 10) | p; d.pad = 0;
                I[ib] = d;
            }
            if (op && ie < want_e) {
                Open o;
                o.x = mx; o.y = my; o.z = mz;
                E[ie] = o;
            }
            nb += __popcll(bb);
            ne += __popcll(be);
        }
        if (lane == 0 && (nb != want_b || ne != want_e)) w.hdr[H_MISMATCH] = 1;     // (every writer stores the same word)
    }
}

__global__ __launch_bounds__(NTT) void shape_trim_kernel(const AbxShapeArgs a, unsigned char* __restrict__ ws) {
    __shared__ double ex[NTT], ey[NTT], ez[NTT];
    __shared__ int wcnt[NWT];
    const int side = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const Workspace w(ws, b, a.L, a.max_dots);
    if (w.skipped()) return;
    const int nI = w.hdr[H_NI + side], nE = w.hdr[H_NE + side];
    Dot* I = w.I + (long long)side * w.M;
    const Open* E = w.E + (long long)side * w.M;
    const double t2 = a.trim * a.trim;
    int kept[1] = {0};
    for (int base = 0; base < nI; base += NTT) {
        const int i = base + tid;
        Dot d;
        d.x = d.y = d.z = 0.0; d.info = d.pad = 0;
        if (i < nI) d = I[i];
        bool keep = i < nI;
        for (int e0 = 0; e0 < nE; e0 += NTT) {
            const int ne = nE - e0 < NTT ? nE - e0 : NTT;
            __syncthreads();                            // the previous chunk has been walked
            if (tid < ne) {
                const Open o = E[e0 + tid];
                ex[tid] = o.x; ey[tid] = o.y; ez[tid] = o.z;
            }
            __syncthreads();
            if (keep)
                for (int e = 0; e < ne; ++e) {
                    const double dx = d.x - ex[e], dy = d.y - ey[e], dz = d.z - ez[e];
                    if ((dx * dx + dy * dy) + dz * dz < t2) {
                        keep = false;
                        break;
                    }
                }
        }
        const unsigned long long bal[1] = {__ballot(keep)};
        int idx[1];
        block_rank<NWT, 1>(bal, wcnt, idx, kept);       // (its first barrier: every dot of this chunk is in registers)
        if (keep) I[idx[0]] = d;                        // in place: idx <= i
    }
    if (tid == 0) w.hdr[H_NT + side] = kept[0];
}

__global__ __launch_bounds__(NT) void shape_match_kernel(const AbxShapeArgs a, unsigned char* __restrict__ ws, int chunk) {
    __shared__ double jx[J_CHUNK], jy[J_CHUNK], jz[J_CHUNK];
    __shared__ int jp[J_CHUNK];
    const int side = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const Workspace w(ws, b, a.L, a.max_dots);
    if (w.skipped()) return;
    const int ni = w.hdr[H_NT + side], nj = w.hdr[H_NT + 1 - side];
    if ((int)blockIdx.x * NT >= ni || nj == 0) return;  // the whole workgroup: no barrier has been passed, the empty list is not read
    const Dot* Ti = w.I + (long long)side * w.M;
    const Dot* Tj = w.I + (long long)(1 - side) * w.M;
    for (int tile = blockIdx.x; tile * NT < ni; tile += gridDim.x) {    // (the same tiles for every thread of the workgroup)
        const int i = tile * NT + tid;
        const bool mine = i < ni;
        double xi = 0.0, yi = 0.0, zi = 0.0;
        int pi = 0;
        if (mine) {
            const Dot d = Ti[i];
            xi = d.x; yi = d.y; zi = d.z; pi = d.info & 1023;
        }
        double best = INFINITY;
        int pj = 0;
        for (int j0 = 0; j0 < nj; j0 += chunk) {
            const int n = nj - j0 < chunk ? nj - j0 : chunk;
            __syncthreads();                            // the previous chunk has been walked
            for (int j = tid; j < n; j += NT) {
                const Dot d = Tj[j0 + j];
                jx[j] = d.x; jy[j] = d.y; jz[j] = d.z; jp[j] = d.info & 1023;
            }
            __syncthreads();
            if (mine)
                for (int j = 0; j < n; ++j) {
                    const double dx = xi - jx[j], dy = yi - jy[j], dz = zi - jz[j];
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < best) {                    // strictly: a tie stays with the lower index
                        best = d2;
                        pj = jp[j];
                    }
                }
        }
        if (mine) {
            const double* ui = a.sphere + 3 * pi;
            const double* uj = a.sphere + 3 * pj;
            const double dot = (ui[0] * uj[0] + ui[1] * uj[1]) + ui[2] * uj[2];
            w.S[(long long)side * w.M + i] = -dot * exp(-(a.weight * best));
            w.D2[(long long)side * w.M + i] = best;
        }
    }
}

// the order of the doubles as unsigned integers
__device__ __forceinline__ unsigned long long to_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_key(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

struct SelectLds {
    int hist[NT];
    int wsum[NW];
    unsigned long long prefix;
    int k;
};

// The k-th smallest (from 0) of v[0..n) - with `region`, of the values whose dot lies in a region row - by a radix select from the top
// byte down.  Called by the whole workgroup with 0 <= k < the number of values; every thread returns the value.
__device__ double select_kth(const double* v, const Dot* dots, const unsigned char* region, int n, int k, SelectLds& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __syncthreads();                                    // the previous result has been read
    if (tid == 0) {
        sh.prefix = 0ull;
        sh.k = k;
    }
    for (int pass = 7; pass >= 0; --pass) {
        sh.hist[tid] = 0;
        __syncthreads();
        const unsigned long long prefix = sh.prefix;
        const int kk = sh.k;
        for (int i = tid; i < n; i += NT) {
            if (region && !region[dots[i].info >> 10]) continue;
            const unsigned long long key = to_key(v[i]);
            const bool match = pass == 7 || (key >> (8 * (pass + 1))) == (prefix >> (8 * (pass + 1)));
            if (match) atomicAdd(&sh.hist[(int)((key >> (8 * pass)) & 255ull)], 1);
        }
        __syncthreads();
        const int h = sh.hist[tid];
        int inc = wave_scan_i(h, lane);
        if (lane == 63) sh.wsum[wv] = inc;
        __syncthreads();                                // (also: every thread has read prefix and k)
        for (int u = 0; u < wv; ++u) inc += sh.wsum[u];
        if (inc - h <= kk && kk < inc) {                // the bin of the k-th value: one thread
            sh.prefix = prefix | ((unsigned long long)tid << (8 * pass));
            sh.k = kk - (inc - h);
        }
        __syncthreads();
    }
    return from_key(sh.prefix);
}

__device__ double median_of(const double* v, const Dot* dots, const unsigned char* region, int n, int count, SelectLds& sh) {
    if (count == 0) return 0.0;
    if (count & 1) return select_kth(v, dots, region, n, (count - 1) / 2, sh);
    const double lo = select_kth(v, dots, region, n, count / 2 - 1, sh), hi = select_kth(v, dots, region, n, count / 2, sh);
    return (lo + hi) * 0.5;
}

__global__ __launch_bounds__(NT) void shape_reduce_kernel(const AbxShapeArgs a, unsigned char* __restrict__ ws) {
    __shared__ SelectLds sh;
    __shared__ int nreg_sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const Workspace w(ws, b, a.L, a.max_dots);
    double* out = a.out + (long long)b * a.out_stride;
    if (w.skipped()) {
        if (tid < ABX_SHAPE_COLS) out[tid] = -1.0;
        return;
    }
    const int nA = w.hdr[H_NT], nB = w.hdr[H_NT + 1];
    const Dot* TA = w.I;
    const Dot* TB = w.I + w.M;
    const double *SA = w.S, *SB = w.S + w.M, *DA = w.D2, *DB = w.D2 + w.M;
    if (tid == 0) nreg_sh = 0;
    __syncthreads();
    int mine = 0;
    if (a.region)
        for (int i = tid; i < nA; i += NT) mine += a.region[TA[i].info >> 10] ? 1 : 0;
    mine = wave_sum_i(mine);
    if ((tid & 63) == 0 && mine) atomicAdd(&nreg_sh, mine);
    __syncthreads();
    const int nreg = nreg_sh;
    const bool both = nA > 0 && nB > 0;                 // without a partner list nothing was matched: S and d2 are not read
    const double sa = both ? median_of(SA, TA, nullptr, nA, nA, sh) : 0.0;
    const double sb = both ? median_of(SB, TB, nullptr, nB, nB, sh) : 0.0;
    const double sr = both && nreg > 0 ? median_of(SA, TA, a.region, nA, nreg, sh) : 0.0;
    const double ga = both ? median_of(DA, TA, nullptr, nA, nA, sh) : 0.0;
    const double gb = both ? median_of(DB, TB, nullptr, nB, nB, sh) : 0.0;
    if (tid == 0) {
        out[0] = (sa + sb) * 0.5;
        out[1] = sa;
        out[2] = sb;
        out[3] = sr;
        out[4] = sqrt(ga);
        out[5] = sqrt(gb);
        out[6] = (double)nA;
        out[7] = (double)nB;
        out[8] = (double)nreg;
        out[9] = (double)(w.hdr[H_NI] - nA);
        out[10] = (double)(w.hdr[H_NI + 1] - nB);
    }
}

}  // namespace

extern "C" long long abx_shape_scores_workspace_bytes(int B, int L, int P, int max_dots) {
    if (B <= 0 || L <= 0 || P <= 0 || max_dots <= 0 || max_dots > MAX_DOTS) return 0;
    return (long long)B * ws_stride(L, max_dots);
}

extern "C" int abx_shape_scores(const AbxShapeArgs* ap, void* workspace, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_shape_scores: null");
    const AbxShapeArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_shape_scores", 1)) return rc;
    ABX_REQUIRE(a.sphere && a.points && a.out && workspace, "abx_shape_scores: null operand");
    ABX_REQUIRE(a.P >= 1 && a.P <= 1024, "abx_shape_scores: P must be in 1..1024");
    ABX_REQUIRE(a.out_stride >= ABX_SHAPE_COLS, "abx_shape_scores: out_stride below ABX_SHAPE_COLS");
    ABX_REQUIRE(std::isfinite(a.probe) && a.probe >= 0.0, "abx_shape_scores: probe must be >= 0");
    ABX_REQUIRE(std::isfinite(a.trim) && a.trim >= 0.0, "abx_shape_scores: trim must be >= 0");
    ABX_REQUIRE(std::isfinite(a.weight) && a.weight >= 0.0, "abx_shape_scores: weight must be >= 0");
    ABX_REQUIRE(a.max_dots >= 1 && a.max_dots <= MAX_DOTS, "abx_shape_scores: max_dots must be in 1..1048576");
    ABX_REQUIRE(a.j_chunk >= 0 && a.j_chunk <= J_CHUNK, "abx_shape_scores: j_chunk must be in 0..1024");
    ABX_REQUIRE(table_lds_bytes(a.L, NWD) <= ABX_LDS_LIMIT, "abx_shape_scores: the atom table does not fit the LDS of a CU (L <= 541)");
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    const int chunk = a.j_chunk ? a.j_chunk : J_CHUNK;
    hipLaunchKernelGGL(shape_offsets_kernel, dim3(a.B), dim3(NT), 0, st, a, ws);
    if (int rc = abx_check_launch("abx_shape_scores(offsets)")) return rc;
    if (int rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(shape_dots_kernel), ABX_LDS_LIMIT, "abx_shape_scores")) return rc;
    hipLaunchKernelGGL(shape_dots_kernel, dim3(DOT_BLOCKS, a.B), dim3(NTD), (int)table_lds_bytes(a.L, NWD), st, a, ws);
    if (int rc = abx_check_launch("abx_shape_scores(dots)")) return rc;
    hipLaunchKernelGGL(shape_trim_kernel, dim3(2, a.B), dim3(NTT), 0, st, a, ws);
    if (int rc = abx_check_launch("abx_shape_scores(trim)")) return rc;
    const int tiles = (a.max_dots + NT - 1) / NT;
    hipLaunchKernelGGL(shape_match_kernel, dim3(tiles < MATCH_TILES ? tiles : MATCH_TILES, 2, a.B), dim3(NT), 0, st, a, ws, chunk);
    if (int rc = abx_check_launch("abx_shape_scores(match)")) return rc;
    hipLaunchKernelGGL(shape_reduce_kernel, dim3(a.B), dim3(NT), 0, st, a, ws);
    return abx_check_launch("abx_shape_scores");
}
