// Ensemble analysis of the N designs of one complex (include/abx_hip.h, AbxEnsemblePairsArgs / AbxEnsembleClusterArgs): what one design
// is to another - RMSD after the optimal proper rotation (shape), RMSD in the complex's frame (placement), differing residues - for
// every pair, and from those planes the Daura / GROMOS clusters and one summary row per design.
//
// Two kernels, no atomics, every sum in a fixed order:
//   ens_pairs_kernel    grid (tile, tile), the upper triangle works.  A workgroup is ONE wave and owns an 8 x 8 tile of (i, j) pairs:
//                       the raw f32 points of its 8 i- and 8 j-structures are staged in LDS (12 P bytes each), one lane per pair.
//                       Centroids per structure (fp64, index order), the 3x3 covariance per pair (fp64, index order), Horn's quaternion
//                       matrix solved PER LANE by cyclic Jacobi rotations on statically indexed registers - the arithmetic of
//                       reduce_dev.h::jacobi4, which survives a degenerate largest eigenvalue (collinear or planar points: any vector of
//                       the eigenspace is optimal), where the adjugate of the characteristic-polynomial route vanishes - and the squared
//                       deviation in a second pass over the points with the rotation found.  i < j is computed, both entries are written.
//                       A pair reads nothing but its two structures: its value does not depend on N or on its tile.
//   ens_cluster_kernel  two workgroups of 1024 threads that share nothing.  Workgroup 0: the adjacency of the clustering plane as a bit
//                       matrix in LDS (row stride odd: lane i reads row i without bank conflicts), per round the unassigned
//                       neighbours by popcount, the arg-max as max of (count << 10 | 1023 - index): most neighbours first, lowest
//                       index on ties, whatever the reduction order.  Workgroup 1: one thread per design, columns 2..9 of its row,
//                       sums over the other designs in index order (reads column i of the symmetric planes: coalesced; the loop
//                       body has no branch, so that eight iterations' loads are in flight at once).
#include "common.h"
#include "abx_hip.h"

namespace {

constexpr int T = 8;                                   // structures per tile side
constexpr int MAXP = ABX_ENS_MAX_POINTS;

__host__ __device__ inline int point_stride(int P) { return (3 * P) | 1; }     // floats per staged structure, odd
inline long long pairs_lds_bytes(int P) { return 2ll * T * point_stride(P) * (long long)sizeof(float); }

// One Jacobi rotation of the symmetric 4x4 matrix A in the (P_, Q_) plane, accumulated in V: reduce_dev.h::jacobi4 with every index a
// compile-time constant, so that both matrices live in registers.
template <int P_, int Q_>
__device__ __forceinline__ void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P_][Q_];
    if (apq == 0.0) return;
    const double theta = (A[Q_][Q_] - A[P_][P_]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][P_], akq = A[k][Q_];
        A[k][P_] = c * akp - sn * akq;
        A[k][Q_] = sn * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = A[P_][k], aqk = A[Q_][k];
        A[P_][k] = c * apk - sn * aqk;
        A[Q_][k] = sn * apk + c * aqk;
    }
    A[P_][Q_] = A[Q_][P_] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P_], vkq = V[k][Q_];
        V[k][P_] = c * vkp - sn * vkq;
        V[k][Q_] = sn * vkp + c * vkq;
    }
}

// The optimal proper rotation R (row major) that moves the centred set a onto the centred set b, from S.jk = sum a_j b_k (Horn 1987:
// the unit quaternion is the eigenvector of the largest eigenvalue of the 4x4 matrix below).  S = 0 gives the identity.
struct Mat3 { double xx, xy, xz, yx, yy, yz, zx, zy, zz; };
__device__ __forceinline__ Mat3 horn_rotation(const Mat3& S) {
    const double Sxx = S.xx, Sxy = S.xy, Sxz = S.xz, Syx = S.yx, Syy = S.yy, Syz = S.yz, Szx = S.zx, Szy = S.zy, Szz = S.zz;
    double A[4][4], V[4][4];
    A[0][0] = Sxx + Syy + Szz; A[0][1] = Syz - Szy;        A[0][2] = Szx - Sxz;         A[0][3] = Sxy - Syx;
    A[1][1] = Sxx - Syy - Szz; A[1][2] = Sxy + Syx;        A[1][3] = Szx + Sxz;
    A[2][2] = -Sxx + Syy - Szz; A[2][3] = Syz + Szy;
    A[3][3] = -Sxx - Syy + Szz;
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) A[i][j] = A[j][i];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 24; ++sweep) {
        double off = 0.0, all = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                all += A[i][j] * A[i][j];
                if (i < j) off += A[i][j] * A[i][j];
            }
        if (off <= 1e-36 * all) break;
        jacobi_rotate<0, 1>(A, V); jacobi_rotate<0, 2>(A, V); jacobi_rotate<0, 3>(A, V);
        jacobi_rotate<1, 2>(A, V); jacobi_rotate<1, 3>(A, V); jacobi_rotate<2, 3>(A, V);
    }
    // the column of the largest eigenvalue by three selects on values.  The empty asm keeps each stage's result in registers: without
    // it the compiler folds the chain into one variable index and parks V in scratch memory to serve it.
    double best = A[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#define ABX_ENS_TAKE(c)                                                                                          \
    {                                                                                                            \
        const bool up = A[c][c] > best;                                                                          \
        best = up ? A[c][c] : best;                                                                              \
        qw = up ? V[0][c] : qw; qx = up ? V[1][c] : qx; qy = up ? V[2][c] : qy; qz = up ? V[3][c] : qz;          \
        asm volatile("" : "+v"(best), "+v"(qw), "+v"(qx), "+v"(qy), "+v"(qz));                                   \
    }
    ABX_ENS_TAKE(1) ABX_ENS_TAKE(2) ABX_ENS_TAKE(3)
#undef ABX_ENS_TAKE
    const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= qn; qx /= qn; qy /= qn; qz /= qn;
    Mat3 R;
    R.xx = 1.0 - 2.0 * (qy * qy + qz * qz); R.xy = 2.0 * (qx * qy - qw * qz);       R.xz = 2.0 * (qx * qz + qw * qy);
    R.yx = 2.0 * (qx * qy + qw * qz);       R.yy = 1.0 - 2.0 * (qx * qx + qz * qz); R.yz = 2.0 * (qy * qz - qw * qx);
    R.zx = 2.0 * (qx * qz - qw * qy);       R.zy = 2.0 * (qy * qz + qw * qx);       R.zz = 1.0 - 2.0 * (qx * qx + qy * qy);
    return R;
}

__global__ __launch_bounds__(64) void ens_pairs_kernel(const AbxEnsemblePairsArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int rows[MAXP];                          // the compared rows, in sequence order
    __shared__ double cen[2 * T][3];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;                                // the lower triangle of tiles is the upper one's transpose
    const int lane = threadIdx.x, N = a.N, M = a.M, P = a.M * a.atoms, stride = point_stride(P);
    float* pts = reinterpret_cast<float*>(lds);         // [2 T][stride]: the i-set, then the j-set
    // ---- the first M set rows of the region below Lpred (missing ones, a caller's miscount, repeat row 0: always in bounds)
    int found = 0;
    for (int base = 0; base < a.Lpred && found < M; base += 64) {
        const int r = base + lane;
        const bool set = r < a.Lpred && a.region[r] != 0;
        const unsigned long long bal = __ballot(set);
        const int rank = found + __popcll(bal & ((1ull << lane) - 1ull));
        if (set && rank < M) rows[rank] = r;
        found += __popcll(bal);
    }
    for (int k = (found < M ? found : M) + lane; k < M; k += 64) rows[k] = 0;
    __syncthreads();
    // ---- stage the points; a structure index beyond N reads the last structure (its pairs are never written)
    auto structure_of = [&](int s) {
        const int g = s < T ? bi * T + s : bj * T + (s - T);
        return g < N ? g : N - 1;
    };
    for (int s = 0; s < 2 * T; ++s) {
        const float* src = a.pred_atom14 + (long long)structure_of(s) * a.pred_sb;
        float* dst = pts + s * stride;
        for (int p = lane; p < P; p += 64) {
            const int m = a.atoms == 1 ? p : p >> 2, slot = a.atoms == 1 ? 1 : p & 3;
            const float* x = src + ((long long)rows[m] * 14 + slot) * 3;
            dst[3 * p] = x[0]; dst[3 * p + 1] = x[1]; dst[3 * p + 2] = x[2];
        }
    }
    __syncthreads();
    // ---- centroid of every staged structure: a property of the structure alone
    if (lane < 2 * T) {
        const float* x = pts + lane * stride;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int p = 0; p < P; ++p) { sx += (double)x[3 * p]; sy += (double)x[3 * p + 1]; sz += (double)x[3 * p + 2]; }
        cen[lane][0] = sx / (double)P; cen[lane][1] = sy / (double)P; cen[lane][2] = sz / (double)P;
    }
    __syncthreads();
    const int ti = lane >> 3, tj = lane & 7;
    const int i = bi * T + ti, j = bj * T + tj;
    const bool pair = i < N && j < N && i < j, diag = i < N && i == j;
    double* fit = a.planes;
    double* frame = a.planes + a.plane_stride;
    double* sdiff = a.planes + 2 * a.plane_stride;
    const long long ij = (long long)i * N + j, ji = (long long)j * N + i;
    if (diag) fit[ij] = frame[ij] = sdiff[ij] = 0.0;
    if (pair) {
        const float* xa = pts + ti * stride;
        const float* xb = pts + (T + tj) * stride;
        const double cax = cen[ti][0], cay = cen[ti][1], caz = cen[ti][2];
        const double cbx = cen[T + tj][0], cby = cen[T + tj][1], cbz = cen[T + tj][2];
        // covariance of the centred sets, and the deviation without superposition
        Mat3 S = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        double d2frame = 0.0;
        for (int p = 0; p < P; ++p) {
            const double rax = (double)xa[3 * p], ray = (double)xa[3 * p + 1], raz = (double)xa[3 * p + 2];
            const double rbx = (double)xb[3 * p], rby = (double)xb[3 * p + 1], rbz = (double)xb[3 * p + 2];
            const double dx = rax - rbx, dy = ray - rby, dz = raz - rbz;
            d2frame += (dx * dx + dy * dy) + dz * dz;
            const double ax = rax - cax, ay = ray - cay, az = raz - caz;
            const double bx = rbx - cbx, by = rby - cby, bz = rbz - cbz;
            S.xx += ax * bx; S.xy += ax * by; S.xz += ax * bz;
            S.yx += ay * bx; S.yy += ay * by; S.yz += ay * bz;
            S.zx += az * bx; S.zy += az * by; S.zz += az * bz;
        }
        const Mat3 R = horn_rotation(S);
        // second pass: the deviation itself with the rotation found (G_a + G_b - 2 lambda cancels for close structures)
        double d2fit = 0.0;
        for (int p = 0; p < P; ++p) {
            const double ax = (double)xa[3 * p] - cax, ay = (double)xa[3 * p + 1] - cay, az = (double)xa[3 * p + 2] - caz;
            const double ex = (R.xx * ax + R.xy * ay + R.xz * az) - ((double)xb[3 * p] - cbx);
            const double ey = (R.yx * ax + R.yy * ay + R.yz * az) - ((double)xb[3 * p + 1] - cby);
            const double ez = (R.zx * ax + R.zy * ay + R.zz * az) - ((double)xb[3 * p + 2] - cbz);
            d2fit += (ex * ex + ey * ey) + ez * ez;
        }
        const double vfit = sqrt(d2fit / (double)P), vframe = sqrt(d2frame / (double)P);
        fit[ij] = vfit; fit[ji] = vfit;
        frame[ij] = vframe; frame[ji] = vframe;
    }
    // ---- the tokens of the compared rows take the place of the points
    __syncthreads();
    long long* tok = reinterpret_cast<long long*>(lds);  // [2 T][M]: 8 M bytes per structure, the points had 12 P >= 12 M
    for (int s = 0; s < 2 * T; ++s) {
        const long long* src = a.pred_seq + (long long)structure_of(s) * a.pred_seq_sb;
        for (int m = lane; m < M; m += 64) tok[s * M + m] = src[rows[m]];
    }
    __syncthreads();
    if (pair) {
        const long long* sa = tok + ti * M;
        const long long* sb = tok + (T + tj) * M;
        int nd = 0;
        for (int m = 0; m < M; ++m) nd += sa[m] != sb[m] ? 1 : 0;
        sdiff[ij] = (double)nd; sdiff[ji] = (double)nd;
    }
}

constexpr int NTC = 1024;                               // threads of a cluster workgroup = ABX_ENS_MAX_N

// Columns 2..9 of the row of design i = threadIdx.x.  Row i of a symmetric plane is read as its column i (consecutive threads,
// consecutive addresses), in index order; the design itself is left out by selects, not by a branch.
__device__ __forceinline__ void summary_row(const AbxEnsembleClusterArgs& a) {
    const int i = threadIdx.x, N = a.N;
    if (i >= N) return;
    const double* fit = a.planes + i;
    const double* frame = a.planes + a.plane_stride + i;
    const double* sdiff = a.planes + 2 * a.plane_stride + i;
    const double inf = __longlong_as_double(0x7ff0000000000000ll), nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool on_fit = a.metric == 0;
    double sfit = 0.0, sframe = 0.0, sseq = 0.0, mfit = inf, mframe = inf;
    int nnb = 0, nsame = 0, first = i;
#pragma unroll 8
    for (int j = 0; j < N; ++j) {
        const long long at = (long long)j * N;
        const double f = fit[at], g = frame[at], s = sdiff[at];
        const bool other = j != i;
        sfit += other ? f : 0.0; sframe += other ? g : 0.0; sseq += other ? s : 0.0;
        mfit = other && f < mfit ? f : mfit;
        mframe = other && g < mframe ? g : mframe;
        nnb += other && (on_fit ? f : g) <= a.cutoff ? 1 : 0;
        const bool same = other && s == 0.0;
        nsame += same ? 1 : 0;
        first = same && j < first ? j : first;
    }
    double* out = a.out + (long long)i * a.out_stride;
    const double n = (double)(N - 1);
    out[2] = (double)nnb;
    out[3] = N > 1 ? sfit / n : nan;    out[4] = N > 1 ? mfit : nan;
    out[5] = N > 1 ? sframe / n : nan;  out[6] = N > 1 ? mframe : nan;
    out[7] = N > 1 ? sseq / n : nan;
    out[8] = (double)nsame;
    out[9] = (double)first;
}

__host__ __device__ inline int adj_words(int N) { return (N + 31) >> 5; }
__host__ __device__ inline int adj_stride(int N) { return adj_words(N) | 1; }
inline long long cluster_lds_bytes(int N) { return (long long)N * adj_stride(N) * 4; }

__global__ __launch_bounds__(NTC) void ens_cluster_kernel(const AbxEnsembleClusterArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    if (blockIdx.x == 1) {                              // the second workgroup: the summary columns
        summary_row(a);
        return;
    }
    __shared__ unsigned un[ABX_ENS_MAX_N / 32];         // designs without a cluster yet
    __shared__ int cen[ABX_ENS_MAX_N];                  // centres in order of discovery
    __shared__ int red[NTC / 64];
    unsigned* adj = reinterpret_cast<unsigned*>(lds);   // [N][WS] neighbour bits
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, N = a.N, W = adj_words(N), WS = adj_stride(N);
    const double* d = a.planes + (long long)a.metric * a.plane_stride;
    // a wave per row, 4 x 64 entries per step (four loads in flight), one ballot per 64: two words of the row's bits
    for (int r = wv; r < N; r += NTC / 64) {
        const double* row = d + (long long)r * N;
        for (int c = 0; c < N; c += 256) {
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = c + 64 * u + lane;
                v[u] = j < N ? row[j] : __longlong_as_double(0x7ff0000000000000ll);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = c + 64 * u + lane, w = (c + 64 * u) >> 5;
                const bool nb = j < N && j != r && v[u] <= a.cutoff;
                const unsigned long long bal = __ballot(nb);
                if (lane == 0 && w < W) {
                    adj[r * WS + w] = (unsigned)bal;
                    if (w + 1 < W) adj[r * WS + w + 1] = (unsigned)(bal >> 32);
                }
            }
        }
    }
    if (tid < W) un[tid] = (tid + 1) * 32 <= N ? 0xffffffffu : (1u << (N - tid * 32)) - 1u;
    int k = 0;
    for (;; ++k) {
        __syncthreads();
        const bool mine = tid < N && ((un[tid >> 5] >> (tid & 31)) & 1u);
        int key = -1;
        if (mine) {
            int cnt = 0;
            for (int w = 0; w < W; ++w) cnt += __popc(adj[tid * WS + w] & un[w]);
            key = (cnt << 10) | (NTC - 1 - tid);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
        if (lane == 0) red[wv] = key;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NTC / 64; ++w) key = max(key, red[w]);
        if (key < 0) break;                             // nobody is left (the same key in every thread)
        const int c = NTC - 1 - (key & (NTC - 1));
        if (mine && (tid == c || ((adj[c * WS + (tid >> 5)] >> (tid & 31)) & 1u))) {
            double* out = a.out + (long long)tid * a.out_stride;
            out[0] = (double)k;
            out[1] = tid == c ? 1.0 : 0.0;
        }
        if (tid == 0) cen[k] = c;
        __syncthreads();                                // every count and membership of this round has been read
        if (tid < W) un[tid] &= ~(adj[c * WS + tid] | (tid == (c >> 5) ? 1u << (c & 31) : 0u));
    }
    if (tid < N) a.centres[tid] = tid < k ? cen[tid] : -1;
    if (tid == 0) a.n_clusters[0] = k;
}

}  // namespace

extern "C" long long abx_ensemble_pairs_workspace_bytes(int N, int P) {
    (void)N; (void)P;
    return 0;
}

extern "C" int abx_ensemble_pairs(const AbxEnsemblePairsArgs* ap, void* workspace, hipStream_t st) {
    (void)workspace;
    ABX_REQUIRE(ap != nullptr, "abx_ensemble_pairs: null");
    const AbxEnsemblePairsArgs a = *ap;
    ABX_REQUIRE(a.N >= 1 && a.N <= 32768, "abx_ensemble_pairs: N must be in 1..32768");
    ABX_REQUIRE(a.atoms == 1 || a.atoms == 4, "abx_ensemble_pairs: atoms must be 1 (C-alpha) or 4 (N, CA, C, O)");
    ABX_REQUIRE(a.M >= 1 && (long long)a.M * a.atoms <= ABX_ENS_MAX_POINTS, "abx_ensemble_pairs: M * atoms must be in 1..ABX_ENS_MAX_POINTS");
    ABX_REQUIRE(a.Lpred >= a.M && a.Lpred < (1 << 22), "abx_ensemble_pairs: Lpred must be in M..2^22");
    ABX_REQUIRE(a.pred_atom14 && a.pred_seq && a.region && a.planes, "abx_ensemble_pairs: null operand");
    ABX_REQUIRE(a.plane_stride >= (long long)a.N * a.N, "abx_ensemble_pairs: plane_stride below N * N");
    const int P = a.M * a.atoms;
    const long long bytes = pairs_lds_bytes(P);
    ABX_REQUIRE(bytes <= ABX_LDS_LIMIT, "abx_ensemble_pairs: the tile does not fit the LDS of a CU");
    if (int rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(ens_pairs_kernel), (int)pairs_lds_bytes(MAXP), "abx_ensemble_pairs")) return rc;
    const int nt = (a.N + T - 1) / T;
    hipLaunchKernelGGL(ens_pairs_kernel, dim3(nt, nt), dim3(64), (int)bytes, st, a);
    return abx_check_launch("abx_ensemble_pairs");
}

extern "C" int abx_ensemble_cluster(const AbxEnsembleClusterArgs* ap, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_ensemble_cluster: null");
    const AbxEnsembleClusterArgs a = *ap;
    ABX_REQUIRE(a.N >= 1 && a.N <= ABX_ENS_MAX_N, "abx_ensemble_cluster: N must be in 1..ABX_ENS_MAX_N");
    ABX_REQUIRE(a.metric == 0 || a.metric == 1, "abx_ensemble_cluster: metric must be 0 (rmsd_fit) or 1 (rmsd_frame)");
    ABX_REQUIRE(a.cutoff >= 0.0, "abx_ensemble_cluster: cutoff must be >= 0");
    ABX_REQUIRE(a.planes && a.out && a.centres && a.n_clusters, "abx_ensemble_cluster: null operand");
    ABX_REQUIRE(a.plane_stride >= (long long)a.N * a.N, "abx_ensemble_cluster: plane_stride below N * N");
    ABX_REQUIRE(a.out_stride >= ABX_ENS_COLS, "abx_ensemble_cluster: out_stride below ABX_ENS_COLS");
    if (int rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(ens_cluster_kernel), (int)cluster_lds_bytes(ABX_ENS_MAX_N), "abx_ensemble_cluster")) return rc;
    hipLaunchKernelGGL(ens_cluster_kernel, dim3(2), dim3(NTC), (int)cluster_lds_bytes(a.N), st, a);
    return abx_check_launch("abx_ensemble_cluster");
}
