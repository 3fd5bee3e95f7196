// Per-pair peptide geometry of the residue pair (l, l + 1), shared by the guidance energies (guidance.hip) and the design scores
// (metrics.hip): the link rule, the flat-bottom term and the three errors of eval/metric_scripts/cal_vio.py:29-110 with their
// gradients.  fp32, one operation per source operation (the build uses -ffp-contract=off): both users get the same bits.
#pragma once
#include <hip/hip_runtime.h>

// row r is peptide-bonded to row r - 1: same chain (full chain ids) and, when residue numbers are given, consecutive numbers
// (a cropped antigen patch or a chain with missing residues keeps one chain id across the gap)
__device__ __forceinline__ bool linked_rows(const int* chain_id, const int* residx, long long r) {
    if (chain_id[r] != chain_id[r - 1]) return false;
    return !residx || residx[r] == residx[r - 1] + 1;
}

// Flat-bottom term relu(sqrt(1e-6 + (v - v0)^2) - tol * sd): returns the energy, `slope` = dE/dv (0 inside the flat bottom)
__device__ __forceinline__ float flat_bottom(float v, float v0, float tol_sd, float& slope) {
    const float err = sqrtf(1e-6f + (v - v0) * (v - v0));
    const float e = err - tol_sd;
    slope = e > 0.f ? (v - v0) / err : 0.f;
    return e > 0.f ? e : 0.f;
}

// g[0..3] receive dE/d(CA_l, C_l, N_u, CA_u) of THIS pair, eb / ea the bond / angle energies; viol: bit 0 / 1 / 2 = the C-N length /
// cos(CA, C, N) / cos(C, N, CA) has left its flat bottom (the reference's violation masks, cal_vio.py:74-75, 93-94, 107-108)
struct PairGrad { float g[4][3]; float eb, ea; int viol; };

// Peptide-geometry terms of one linked pair whose C_l and N_u exist (eval/metric_scripts/cal_vio.py:29-110): the C-N bond length and
// the cosines of the CA-C-N and C-N-CA angles against their literature values (abx/common/residue_constants.py:475-480), each a
// flat-bottom violation.  ca / c: CA, C of the lower residue; n / ca2: N, CA of the upper one (m_ca / m_ca2: the CA exists);
// pro: the upper residue is a proline.  `o` arrives zeroed; w_angle == 0 skips the angle terms.
__device__ __forceinline__ void peptide_terms(const float* ca, const float* c, const float* n, const float* ca2, bool m_ca, bool m_ca2,
                                              bool pro, float w_bond, float w_angle, float tolerance_factor, PairGrad& o) {
    const float l0 = pro ? 1.341f : 1.329f, sd = pro ? 0.016f : 0.014f;
    // ---- bond: v = |C - N|
    const float bx = n[0] - c[0], by = n[1] - c[1], bz = n[2] - c[2];           // C -> N
    const float d = sqrtf(1e-6f + bx * bx + by * by + bz * bz);
    float sl;
    const float fb = flat_bottom(d, l0, tolerance_factor * sd, sl);
    o.eb = w_bond * fb;
    o.viol |= fb > 0.f ? 1 : 0;
    {
        const float s = w_bond * sl / d;                                        // dE/dN = s * (N - C)
        o.g[2][0] += s * bx; o.g[2][1] += s * by; o.g[2][2] += s * bz;
        o.g[1][0] -= s * bx; o.g[1][1] -= s * by; o.g[1][2] -= s * bz;
    }
    if (w_angle == 0.f) return;
    // unit vector C -> N (l2_normalize: x / sqrt(max(|x|^2, 1e-12)), abx/model/utils.py:12-14)
    const float nb = sqrtf(fmaxf(bx * bx + by * by + bz * bz, 1e-12f));
    const float vx = bx / nb, vy = by / nb, vz = bz / nb;
    // cos(x, y) of unit vectors u = p / |p|, v = q / |q| about a vertex: d cos / dp = (v - cos u) / |p|, d cos / dq = (u - cos v) / |q|
    if (m_ca) {     // ---- CA_l - C_l - N_u  (vertex C): p = CA - C, q = N - C
        const float px = ca[0] - c[0], py = ca[1] - c[1], pz = ca[2] - c[2];
        const float np_ = sqrtf(fmaxf(px * px + py * py + pz * pz, 1e-12f));
        const float ux = px / np_, uy = py / np_, uz = pz / np_;
        const float cs = ux * vx + uy * vy + uz * vz;
        const float e = flat_bottom(cs, -0.4473f, tolerance_factor * 0.0311f, sl);
        o.ea += w_angle * e;
        o.viol |= e > 0.f ? 2 : 0;
        const float k = w_angle * sl;
        const float gp[3] = {k * (vx - cs * ux) / np_, k * (vy - cs * uy) / np_, k * (vz - cs * uz) / np_};
        const float gq[3] = {k * (ux - cs * vx) / nb, k * (uy - cs * vy) / nb, k * (uz - cs * vz) / nb};
#pragma unroll
        for (int x = 0; x < 3; ++x) { o.g[0][x] += gp[x]; o.g[2][x] += gq[x]; o.g[1][x] -= gp[x] + gq[x]; }
    }
    if (m_ca2) {    // ---- C_l - N_u - CA_u  (vertex N): p = C - N = -b, q = CA_u - N
        const float qx = ca2[0] - n[0], qy = ca2[1] - n[1], qz = ca2[2] - n[2];
        const float nq = sqrtf(fmaxf(qx * qx + qy * qy + qz * qz, 1e-12f));
        const float wx = qx / nq, wy = qy / nq, wz = qz / nq;
        const float ux = -vx, uy = -vy, uz = -vz;
        const float cs = ux * wx + uy * wy + uz * wz;
        const float e = flat_bottom(cs, -0.5203f, tolerance_factor * 0.0353f, sl);
        o.ea += w_angle * e;
        o.viol |= e > 0.f ? 4 : 0;
        const float k = w_angle * sl;
        const float gp[3] = {k * (wx - cs * ux) / nb, k * (wy - cs * uy) / nb, k * (wz - cs * uz) / nb};
        const float gq[3] = {k * (ux - cs * wx) / nq, k * (uy - cs * wy) / nq, k * (uz - cs * wz) / nq};
#pragma unroll
        for (int x = 0; x < 3; ++x) { o.g[1][x] += gp[x]; o.g[3][x] += gq[x]; o.g[2][x] -= gp[x] + gq[x]; }
    }
}
