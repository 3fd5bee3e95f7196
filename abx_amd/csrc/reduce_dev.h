// Wave and block helpers of the per-design analyses: fixed-order sums (metrics, accuracy, interface, torsions), ballot ranks over a
// block (metrics, interface, polar, developability, shape), lds_add (developability, patches) and the superposition by Horn's
// quaternion (metrics, accuracy).  ensemble.hip is not a user: its Jacobi is a register-resident formulation of its own with another
// rotation order, and its results are pinned bit for bit by the ensemble tests.
#pragma once
#include "common.h"

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// number of set bits of a ballot below this lane
__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ int wave_scan_i(int v, int lane) {       // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        v += lane >= o ? t : 0;
    }
    return v;
}

// N integer columns over the NW waves of the block, chunk after chunk: `total` runs over the calls (zero before the first one).
// before[k] grows by total[k] on entry + the totals of the waves below this thread's (the caller puts the thread's place in its own
// wave there); total[k] grows by those of all waves.
// wave_totals[k] is read from lane 63 of every wave (the last lane of an inclusive scan; a popcount of a ballot is the same in every
// lane).  Called by every thread of the block: two barriers, the first one frees `sh` ([NW][N] ints) from its previous use.
template <int NW, int N>
__device__ __forceinline__ void block_offsets(const int (&wave_totals)[N], int* sh, int (&before)[N], int (&total)[N]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < N; ++k) sh[wv * N + k] = wave_totals[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) before[k] += total[k];
#pragma nounroll                                        // (unrolled, the NW * N loads are in flight at once: 7 VGPRs more at N = 6)
    for (int u = 0; u < NW; ++u) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int c = sh[u * N + k];
            before[k] += u < wv ? c : 0;
            total[k] += c;
        }
    }
}

// rank[k] = total[k] on entry + the set bits of ballot k in the lanes and waves of the block below this thread; total[k] grows by all
// of them.  As block_offsets.
template <int NW, int N>
__device__ __forceinline__ void block_rank(const unsigned long long (&ballots)[N], int* sh, int (&rank)[N], int (&total)[N]) {
    int wave_totals[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        wave_totals[k] = __popcll(ballots[k]);
        rank[k] = lanes_below(ballots[k]);
    }
    block_offsets<NW, N>(wave_totals, sh, rank, total);
}

// a signed 64-bit sum in LDS (two's complement)
__device__ __forceinline__ void lds_add(unsigned long long* p, long long v) { atomicAdd(p, (unsigned long long)v); }

// Sum of N doubles per thread over the 256 threads of the block, in a fixed order; every thread returns with the totals in v.
// `sh`: [4][N] doubles.
template <int N>
__device__ __forceinline__ void block_sum_d(double (&v)[N], double* sh) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum_d(v[k]);
    __syncthreads();                                   // the previous use of sh is over
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sh[(tid >> 6) * N + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (sh[k] + sh[N + k]) + (sh[2 * N + k] + sh[3 * N + k]);
}

// Eigenvectors of the symmetric 4x4 matrix A (LDS) by cyclic Jacobi rotations, accumulated in V (LDS).  One thread.  A rotation
// zeroes A[p][q] exactly; the sweeps stop when the off-diagonal mass is below 1e-36 of the matrix (quadratic convergence: 5-7 sweeps).
__device__ inline void jacobi4(double (*A)[4], double (*V)[4]) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 24; ++sweep) {
        double off = 0.0, all = 0.0;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                all += A[i][j] * A[i][j];
                if (i < j) off += A[i][j] * A[i][j];
            }
        if (off <= 1e-36 * all) break;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - sn * akq;
                    A[k][q] = sn * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - sn * aqk;
                    A[q][k] = sn * apk + c * aqk;
                }
                A[p][q] = A[q][p] = 0.0;
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - sn * vkq;
                    V[k][q] = sn * vkp + c * vkq;
                }
            }
    }
}

// The optimal proper rotation of the covariance S[j][k] = sum (g_j - cg_j)(p_k - cp_k), row-major into Rs[9] (LDS).  Horn 1987: its
// unit quaternion is the eigenvector of the largest eigenvalue of N.  One thread; Nm and Vm are LDS so that no index is a register index.
__device__ __forceinline__ void horn_rotation_lds(const double (&S)[9], double (*Nm)[4], double (*Vm)[4], double* Rs) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    Nm[0][0] = Sxx + Syy + Szz; Nm[0][1] = Syz - Szy;       Nm[0][2] = Szx - Sxz;        Nm[0][3] = Sxy - Syx;
    Nm[1][1] = Sxx - Syy - Szz; Nm[1][2] = Sxy + Syx;       Nm[1][3] = Szx + Sxz;
    Nm[2][2] = -Sxx + Syy - Szz; Nm[2][3] = Syz + Szy;
    Nm[3][3] = -Sxx - Syy + Szz;
    for (int i = 1; i < 4; ++i)
        for (int j = 0; j < i; ++j) Nm[i][j] = Nm[j][i];
    jacobi4(Nm, Vm);
    int im = 0;
    for (int i = 1; i < 4; ++i)
        if (Nm[i][i] > Nm[im][im]) im = i;
    double qw = Vm[0][im], qx = Vm[1][im], qy = Vm[2][im], qz = Vm[3][im];
    const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= qn; qx /= qn; qy /= qn; qz /= qn;
    Rs[0] = 1.0 - 2.0 * (qy * qy + qz * qz); Rs[1] = 2.0 * (qx * qy - qw * qz);       Rs[2] = 2.0 * (qx * qz + qw * qy);
    Rs[3] = 2.0 * (qx * qy + qw * qz);       Rs[4] = 1.0 - 2.0 * (qx * qx + qz * qz); Rs[5] = 2.0 * (qy * qz - qw * qx);
    Rs[6] = 2.0 * (qx * qz - qw * qy);       Rs[7] = 2.0 * (qy * qz + qw * qx);       Rs[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
}
