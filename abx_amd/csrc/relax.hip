// Violation relaxation of designed residues (include/abx_hip.h, AbxRelaxArgs): steepest descent with an adaptive step on the
// violation energy of guidance.hip restricted to the terms that touch a movable residue, in the space of rigid-body motions of every
// movable residue plus its side-chain chi angles.  The whole minimisation of one structure is ONE workgroup of one launch:
//
//   stage     the atom table of the structure (position + radius of all 14 L atom slots as float4, chain id and link / movable /
//             residue-type bits per row) goes into LDS once; the movable rows are compacted into a list.
//   evaluate  (a) rebuild: one thread per movable residue turns (t, q, chi) and the INPUT coordinates into positions, in place in
//                 the LDS atom table (the chi rotations read their axis atoms from there: no register arrays, no scratch);
//             (b) pairs: 16 lanes share one movable atom and walk the atom table in steps of 16 slots (consecutive float4 per
//                 group, the same address in all four groups of a wave: conflict-free broadcast reads); the force on the atom is
//                 summed over the 16 lanes with xor shuffles, the energy per thread in fp64;
//             (c) one thread per movable residue adds the peptide terms (peptide_dev.h) of the pairs (i - 1, i), (i, i + 1) to
//                 its backbone atoms, the restraint, and pulls the atom gradients back to (g_t, tau, g_chi);
//             (d) the four energies are summed over the block in a fixed order (wave shuffles, then 16 partials from LDS).
//   decide    every thread compares the same two fp64 numbers: accept (swap state pointers, eta *= grow) or drop (eta *= shrink).
//
// Block barriers separate (a) / (b) / (c) / (d); there is no atomic, no spin-wait and no communication between workgroups, and the
// loop runs at most max_iter times.  A structure's result depends on nothing but its own inputs.
//
// What fits: 232 L + 340 M + 1024 bytes of LDS <= 160 KB (abx_relax_lds_bytes; L = 352 with M <= 238).  A larger problem is an
// argument error (abx_last_error_string), there is no global-memory path for the atom table.
#include "common.h"
#include "abx_hip.h"
#include "peptide_dev.h"
#include "structure_dev.h"

namespace {

constexpr int NT = 1024;               // threads per workgroup
constexpr int GS = 16;                 // lanes that share one movable atom
constexpr int NG = NT / GS;            // movable atoms per pass
constexpr int NW = NT / 64;            // waves

__host__ __device__ constexpr long long lds_bytes(int L, int M) { return 232ll * L + 340ll * M + 1024; }

using Structure = StructureView<AbxRelaxArgs>;      // (the complex is shared by the batch)

// rinfo bits of a row
constexpr int R_LINK = 1, R_MOV = 2, R_CYS = 4, R_AA_SHIFT = 8;

// The peptide terms of the row pair (l, l + 1) from the LDS atom table: zero when the pair is not linked or its C / N is missing
__device__ __forceinline__ void peptide_pair(const AbxRelaxArgs& a, const float4* env, const int* rinfo, int l, PairGrad& o) {
#pragma unroll
    for (int k = 0; k < 4; ++k) o.g[k][0] = o.g[k][1] = o.g[k][2] = 0.f;
    o.eb = o.ea = 0.f;
    o.viol = 0;
    if (l < 0 || l + 1 >= a.L || !(rinfo[l + 1] & R_LINK)) return;
    const float4* lo = env + l * 14;
    const float4* up = env + (l + 1) * 14;
    if (lo[2].w < 0.f || up[0].w < 0.f) return;
    peptide_terms(&lo[1].x, &lo[2].x, &up[0].x, &up[1].x, lo[1].w >= 0.f, up[1].w >= 0.f, (rinfo[l + 1] >> R_AA_SHIFT) == 14, a.w_bond,
                  a.w_angle, a.bond_tolerance_factor, o);
}

__global__ __launch_bounds__(NT) void relax_kernel(const AbxRelaxArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int L = a.L, M = a.M, tid = threadIdx.x, b = blockIdx.x;
    float4* env = reinterpret_cast<float4*>(lds);                      // [14 L]: x, y, z, radius (< 0: the atom does not exist)
    double* red = reinterpret_cast<double*>(lds + 224ll * L);          // [NW][4]
    int* ctl = reinterpret_cast<int*>(red + NW * 4);                   // [16]: 0 = movable rows found, 1 = largest radius (float bits)
    int* chn = ctl + 16;                                               // [L] chain id
    int* rinfo = chn + L;                                              // [L] R_* bits | residue type << 8
    int* mrow = rinfo + L;                                             // [M] row of every movable residue
    float* S = reinterpret_cast<float*>(mrow + M);                     // [M][11] accepted state: t, q (w, x, y, z), chi
    float* St = S + 11 * M;                                            // [M][11] trial state
    float* G = St + 11 * M;                                            // [M][10] generalised gradient at S: g_t, tau, g_chi
    float* Gt = G + 10 * M;                                            // [M][10] ... at St
    float* gA = Gt + 10 * M;                                           // [M][14][3] atom gradients of the movable residues
    const Structure s(a, b);

    // ---- stage
    for (int j = tid; j < L * 14; j += NT) {
        const int res = j / 14, slot = j - res * 14;
        const int aa = s.aatype(res);
        const float* x = s.xyz(res, slot);
        env[j] = make_float4(x[0], x[1], x[2], s.exists(res, slot, aa) ? s.radius[aa * 14 + slot] : -1.f);
    }
    for (int r = tid; r < L; r += NT) {
        const int aa = s.aatype(r);
        const bool link = r > 0 && linked_rows(a.chain_id, a.residx, r);
        const bool mov = r < a.Lpred && a.movable[r] != 0;
        chn[r] = a.chain_id[r];
        rinfo[r] = (link ? R_LINK : 0) | (mov ? R_MOV : 0) | (aa == 4 ? R_CYS : 0) | (aa << R_AA_SHIFT);
    }
    if (tid < 64) {
        float rm = 0.f;
        for (int k = tid; k < 21 * 14; k += 64) rm = fmaxf(rm, a.radius[k]);
        rm = wave_max(rm);
        if (tid == 0) ctl[1] = __float_as_int(rm);
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int r = 0; r < L; ++r) {
            if (!(rinfo[r] & R_MOV)) continue;
            if (n < M) mrow[n++] = r;
            else rinfo[r] &= ~R_MOV;                                   // beyond the caller's count: a fixed row
        }
        ctl[0] = n;
    }
    for (int m = tid; m < M; m += NT) {
        float* o = S + m * 11;
#pragma unroll
        for (int k = 0; k < 11; ++k) o[k] = k == 3 ? 1.f : 0.f;
    }
    __syncthreads();
    const int Mu = ctl[0];
    const float rmax = __int_as_float(ctl[1]);
    const float rho2 = a.rho * a.rho;

    // positions of the movable residues from a state (one thread per residue, in place in the atom table)
    auto rebuild = [&](const float* state) {
        for (int m = tid; m < Mu; m += NT) {
            const float* st = state + m * 11;
            const int i = mrow[m], aa = rinfo[i] >> R_AA_SHIFT;
            float4* e = env + i * 14;
            const float* xin = s.xyz(i, 0);
            const float cx = xin[3], cy = xin[4], cz = xin[5];          // input C-alpha
            for (int k = 0; k < 14; ++k) {
                e[k].x = xin[3 * k] - cx; e[k].y = xin[3 * k + 1] - cy; e[k].z = xin[3 * k + 2] - cz;
            }
            for (int c = 0; c < 4; ++c) {
                const int a1 = a.chi_axis[(aa * 4 + c) * 2], a2 = a.chi_axis[(aa * 4 + c) * 2 + 1];
                const float ang = st[7 + c];
                if (a1 < 0 || ang == 0.f || e[a1].w < 0.f || e[a2].w < 0.f) continue;
                const float px = e[a2].x, py = e[a2].y, pz = e[a2].z;
                float ux = px - e[a1].x, uy = py - e[a1].y, uz = pz - e[a1].z;
                const float un = sqrtf(ux * ux + uy * uy + uz * uz + 1e-30f);
                ux /= un; uy /= un; uz /= un;
                float cs = __cosf(ang), sn = __sinf(ang);
                const float nn = sqrtf(cs * cs + sn * sn);
                cs /= nn; sn /= nn;
                for (int k = 5; k < 14; ++k) {                          // slots 0-4 (N, CA, C, O, CB) belong to no chi group
                    if (a.rigid_group[aa * 14 + k] < 4 + c) continue;
                    const float vx = e[k].x - px, vy = e[k].y - py, vz = e[k].z - pz;
                    const float dt = (ux * vx + uy * vy + uz * vz) * (1.f - cs);
                    e[k].x = (vx * cs + (uy * vz - uz * vy) * sn + ux * dt) + px;
                    e[k].y = (vy * cs + (uz * vx - ux * vz) * sn + uy * dt) + py;
                    e[k].z = (vz * cs + (ux * vy - uy * vx) * sn + uz * dt) + pz;
                }
            }
            const float qw = st[3], qx = st[4], qy = st[5], qz = st[6];
            const float r00 = 1.f - 2.f * (qy * qy + qz * qz), r01 = 2.f * (qx * qy - qw * qz), r02 = 2.f * (qx * qz + qw * qy);
            const float r10 = 2.f * (qx * qy + qw * qz), r11 = 1.f - 2.f * (qx * qx + qz * qz), r12 = 2.f * (qy * qz - qw * qx);
            const float r20 = 2.f * (qx * qz - qw * qy), r21 = 2.f * (qy * qz + qw * qx), r22 = 1.f - 2.f * (qx * qx + qy * qy);
            const float ox = cx + st[0], oy = cy + st[1], oz = cz + st[2];
            for (int k = 0; k < 14; ++k) {
                const float vx = e[k].x, vy = e[k].y, vz = e[k].z;
                e[k].x = (r00 * vx + r01 * vy + r02 * vz) + ox;
                e[k].y = (r10 * vx + r11 * vy + r12 * vz) + oy;
                e[k].z = (r20 * vx + r21 * vy + r22 * vz) + oz;
            }
        }
    };

    double Ecur[4] = {0, 0, 0, 0}, E0[3] = {0, 0, 0}, E = 0.0;
    float eta = a.eta0;
    int n = 0, acc = 0;
    bool env_is_current = true;
    const int grp = tid / GS, ln = tid % GS;
    for (;;) {
        if (n > 0) {
            // ---- trial state: one step down the generalised gradient
            for (int m = tid; m < Mu; m += NT) {
                const float* st = S + m * 11;
                const float* g = G + m * 10;
                float* o = St + m * 11;
                o[0] = st[0] - eta * g[0]; o[1] = st[1] - eta * g[1]; o[2] = st[2] - eta * g[2];
                const float wx = -eta * g[3] / rho2, wy = -eta * g[4] / rho2, wz = -eta * g[5] / rho2;
                const float th = sqrtf(wx * wx + wy * wy + wz * wz);
                float hs = 0.5f, dw = 1.f;                              // dq = (cos(th / 2), sin(th / 2) w / th)
                if (th > 1e-6f) { hs = __sinf(0.5f * th) / th; dw = __cosf(0.5f * th); }
                const float dx = hs * wx, dy = hs * wy, dz = hs * wz;
                const float qw = st[3], qx = st[4], qy = st[5], qz = st[6];
                float nw = dw * qw - (dx * qx + dy * qy + dz * qz);
                float nx = dw * qx + qw * dx + (dy * qz - dz * qy);
                float ny = dw * qy + qw * dy + (dz * qx - dx * qz);
                float nz = dw * qz + qw * dz + (dx * qy - dy * qx);
                const float qn = sqrtf(nw * nw + nx * nx + ny * ny + nz * nz);
                o[3] = nw / qn; o[4] = nx / qn; o[5] = ny / qn; o[6] = nz / qn;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[7 + c] = st[7 + c] - eta * g[6 + c] / rho2;
            }
            rebuild(St);
            __syncthreads();
        }
        // ---- (b) atom pairs with a movable atom
        double ec = 0.0;
        for (int base = 0; base < Mu * 14; base += NG) {
            const int ai = base + grp;
            float gx = 0.f, gy = 0.f, gz = 0.f;
            if (ai < Mu * 14) {
                const int m = ai / 14, ms = ai - m * 14, mres = mrow[m];
                const float4 me = env[mres * 14 + ms];
                if (me.w > 0.f) {
                    const int minfo = rinfo[mres], mchain = chn[mres];
                    const bool mlink = (minfo & R_LINK) != 0, msg = (minfo & R_CYS) && ms == 5;
                    // no pair beyond this distance can overlap: r_a + r_b - tolerance <= cm (with a margin far above fp32 rounding)
                    const float cm = me.w + rmax - a.overlap_tolerance;
                    const float cut2 = cm > 0.f ? cm * cm * 1.001f + 1e-3f : -1.f;
                    int r = ln / 14, sl = ln - r * 14;
                    for (int j = ln; j < L * 14; j += GS) {
                        const float4 o = env[j];
                        if (o.w > 0.f && r != mres) {
                            const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
                            if (dx * dx + dy * dy + dz * dz <= cut2) {
                                const int oinfo = rinfo[r];
                                // peptide bond C(i) - N(i+1) of linked neighbours, SG - SG disulfide
                                const bool excl = (r == mres + 1 && ms == 2 && sl == 0 && (oinfo & R_LINK)) ||
                                                  (mres == r + 1 && sl == 2 && ms == 0 && mlink) || (msg && (oinfo & R_CYS) && sl == 5);
                                if (!excl) {
                                    // the overlap of guidance.hip::clash_kernel, operation for operation
                                    const float d = sqrtf(1e-10f + dx * dx + dy * dy + dz * dz);
                                    const float ov = me.w + o.w - a.overlap_tolerance - d;
                                    if (ov > 0.f) {
                                        const float w = (chn[r] == mchain ? 1.0f : a.between_chain_factor) * a.w_clash;
                                        // a pair of two movable atoms is visited from both of them
                                        ec += (double)((oinfo & R_MOV) ? 0.5f * w * ov : w * ov);
                                        const float sc = -w / d;
                                        gx += sc * dx; gy += sc * dy; gz += sc * dz;
                                    }
                                }
                            }
                        }
                        sl += GS - 14; r += 1;
                        if (sl >= 14) { sl -= 14; r += 1; }
                    }
                }
            }
#pragma unroll
            for (int o = GS / 2; o > 0; o >>= 1) {
                gx += __shfl_xor(gx, o, 64); gy += __shfl_xor(gy, o, 64); gz += __shfl_xor(gz, o, 64);
            }
            if (ln == 0 && ai < Mu * 14) { gA[ai * 3] = gx; gA[ai * 3 + 1] = gy; gA[ai * 3 + 2] = gz; }
        }
        __syncthreads();
        // ---- (c) peptide terms, restraint, pull-back to the degrees of freedom of the residue
        double eb = 0.0, ea = 0.0, er = 0.0;
        for (int m = tid; m < Mu; m += NT) {
            const int i = mrow[m], aa = rinfo[i] >> R_AA_SHIFT;
            const float4* e = env + i * 14;
            float* g = gA + m * 42;
            PairGrad lo, hi;
            peptide_pair(a, env, rinfo, i - 1, lo);                     // this residue is the upper one: N (g[2]), CA (g[3])
            peptide_pair(a, env, rinfo, i, hi);                         // this residue is the lower one: CA (g[0]), C (g[1])
            const bool lo_mine = !(i > 0 && (rinfo[i - 1] & R_MOV));    // a pair of two movable residues is counted by the lower one
            eb += (double)hi.eb + (lo_mine ? (double)lo.eb : 0.0);
            ea += (double)hi.ea + (lo_mine ? (double)lo.ea : 0.0);
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                g[x] += lo.g[2][x];
                g[3 + x] += lo.g[3][x] + hi.g[0][x];
                g[6 + x] += hi.g[1][x];
            }
            const float* xin = s.xyz(i, 1);
            const float px = e[1].x, py = e[1].y, pz = e[1].z;          // the pivot: the C-alpha slot
            const float rx = px - xin[0], ry = py - xin[1], rz = pz - xin[2];
            er += (double)(a.k_restraint * (rx * rx + ry * ry + rz * rz));
            float ft[3] = {2.f * a.k_restraint * rx, 2.f * a.k_restraint * ry, 2.f * a.k_restraint * rz}, tq[3] = {0.f, 0.f, 0.f};
            for (int k = 0; k < 14; ++k) {
                if (e[k].w < 0.f) continue;
                const float vx = e[k].x - px, vy = e[k].y - py, vz = e[k].z - pz;
                const float g0 = g[3 * k], g1 = g[3 * k + 1], g2 = g[3 * k + 2];
                ft[0] += g0; ft[1] += g1; ft[2] += g2;
                tq[0] += vy * g2 - vz * g1;
                tq[1] += vz * g0 - vx * g2;
                tq[2] += vx * g1 - vy * g0;
            }
            float* o = Gt + m * 10;
            o[0] = ft[0]; o[1] = ft[1]; o[2] = ft[2]; o[3] = tq[0]; o[4] = tq[1]; o[5] = tq[2];
            for (int c = 0; c < 4; ++c) {
                const int a1 = a.chi_axis[(aa * 4 + c) * 2], a2 = a.chi_axis[(aa * 4 + c) * 2 + 1];
                float gc = 0.f;
                if (a1 >= 0 && e[a1].w >= 0.f && e[a2].w >= 0.f) {
                    const float qx = e[a2].x, qy = e[a2].y, qz = e[a2].z;
                    float ux = qx - e[a1].x, uy = qy - e[a1].y, uz = qz - e[a1].z;
                    const float un = sqrtf(ux * ux + uy * uy + uz * uz + 1e-30f);
                    ux /= un; uy /= un; uz /= un;
                    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
                    for (int k = 5; k < 14; ++k) {
                        if (e[k].w < 0.f || a.rigid_group[aa * 14 + k] < 4 + c) continue;
                        const float vx = e[k].x - qx, vy = e[k].y - qy, vz = e[k].z - qz;
                        const float g0 = g[3 * k], g1 = g[3 * k + 1], g2 = g[3 * k + 2];
                        t0 += vy * g2 - vz * g1;
                        t1 += vz * g0 - vx * g2;
                        t2 += vx * g1 - vy * g0;
                    }
                    gc = ux * t0 + uy * t1 + uz * t2;
                }
                o[6 + c] = gc;
            }
        }
        // ---- (d) the energies of the block, fixed order
        ec = wave_sum_d(ec); eb = wave_sum_d(eb); ea = wave_sum_d(ea); er = wave_sum_d(er);
        if ((tid & 63) == 0) {
            double* o = red + (tid >> 6) * 4;
            o[0] = ec; o[1] = eb; o[2] = ea; o[3] = er;
        }
        __syncthreads();
        double Et[4] = {0, 0, 0, 0};
        for (int w = 0; w < NW; ++w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) Et[k] += red[w * 4 + k];
        }
        const double Etr = ((Et[0] + Et[1]) + Et[2]) + Et[3];
        ++n;
        bool take;
        if (n == 1) {
            take = true;
            E0[0] = Et[0]; E0[1] = Et[1]; E0[2] = Et[2];
        } else {
            take = Etr < E;
            if (take) { eta *= a.grow; ++acc; float* t = S; S = St; St = t; }
            else eta *= a.shrink;
            env_is_current = take;
        }
        if (take) {
            E = Etr;
#pragma unroll
            for (int k = 0; k < 4; ++k) Ecur[k] = Et[k];
            float* t = G; G = Gt; Gt = t;
        }
        // (the next write of `red` lies behind two more barriers; S / St / G / Gt rows are touched by their own thread only)
        if (n >= a.max_iter || E == 0.0) break;
    }
    // ---- the returned structure
    if (acc > 0 && !env_is_current) rebuild(S);                         // (every read of the dropped trial lies before barrier (d))
    __syncthreads();
    float dmax = 0.f;
    if (acc > 0) {
        for (int m = tid; m < Mu; m += NT) {
            const int i = mrow[m];
            const float* xin = s.xyz(i, 1);
            const float4 c = env[i * 14 + 1];
            const float rx = c.x - xin[0], ry = c.y - xin[1], rz = c.z - xin[2];
            dmax = fmaxf(dmax, sqrtf(rx * rx + ry * ry + rz * rz));
        }
    }
    dmax = wave_max(dmax);
    if ((tid & 63) == 0) red[tid >> 6] = (double)dmax;                  // (every thread has left the loop: `red` is free)
    float* out = a.out_atom14 + (long long)b * a.out_sb;
    for (int j = tid; j < a.Lpred * 14; j += NT) {
        const int res = j / 14;
        const float4 p = env[j];
        const float* x = s.pred + (long long)j * 3;
        const bool moved = acc > 0 && (rinfo[res] & R_MOV) && p.w >= 0.f;
        out[3 * j] = moved ? p.x : x[0];
        out[3 * j + 1] = moved ? p.y : x[1];
        out[3 * j + 2] = moved ? p.z : x[2];
    }
    if (a.gen_grad) {
        float* gg = a.gen_grad + (long long)b * M * 10;
        for (int k = tid; k < M * 10; k += NT) gg[k] = k < Mu * 10 ? G[k] : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        double dm = 0.0;
        for (int w = 0; w < NW; ++w) dm = red[w] > dm ? red[w] : dm;
        double* o = a.report + (long long)b * a.report_stride;
        o[0] = E0[0]; o[1] = E0[1]; o[2] = E0[2];
        o[3] = Ecur[0]; o[4] = Ecur[1]; o[5] = Ecur[2]; o[6] = Ecur[3];
        o[7] = (double)n; o[8] = (double)acc; o[9] = (double)eta; o[10] = dm;
    }
}

}  // namespace

extern "C" long long abx_relax_lds_bytes(int L, int M) {
    if (L <= 0 || M < 0) return 0;
    return lds_bytes(L, M);
}

// The atom table lives in LDS: nothing is needed today (the argument is the place of a global-memory table for larger problems)
extern "C" long long abx_relax_workspace_bytes(int B, int L, int M) {
    (void)B; (void)L; (void)M;
    return 0;
}

extern "C" int abx_relax(const AbxRelaxArgs* ap, void* workspace, hipStream_t st) {
    (void)workspace;
    ABX_REQUIRE(ap != nullptr, "abx_relax: null");
    const AbxRelaxArgs a = *ap;
    if (int rc = abx_check_structure_args(a, "abx_relax", 2)) return rc;
    ABX_REQUIRE(a.M > 0 && a.M <= a.Lpred, "abx_relax: M (movable residues) must be in 1..Lpred");
    ABX_REQUIRE(lds_bytes(a.L, a.M) <= ABX_LDS_LIMIT, "abx_relax: the structure does not fit the LDS-resident atom table (232 L + 340 M + 1024 bytes > 160 KB)");
    ABX_REQUIRE(a.chain_id && a.movable && a.chi_axis && a.rigid_group && a.out_atom14 && a.report, "abx_relax: null operand");
    ABX_REQUIRE(a.out_sb >= (long long)a.Lpred * 42 && a.report_stride >= ABX_RELAX_COLS, "abx_relax: out_sb below Lpred * 42 or report_stride below ABX_RELAX_COLS");
    ABX_REQUIRE(a.max_iter >= 0 && a.eta0 > 0.f && a.rho > 0.f && a.grow >= 1.f && a.shrink > 0.f && a.shrink < 1.f && a.k_restraint >= 0.f,
                "abx_relax: bad parameters (max_iter >= 0, eta0 > 0, rho > 0, grow >= 1, 0 < shrink < 1, k_restraint >= 0)");
    const int bytes = (int)lds_bytes(a.L, a.M);
    if (int rc = abx_ensure_dynamic_lds(reinterpret_cast<const void*>(relax_kernel), ABX_LDS_LIMIT, "abx_relax")) return rc;
    hipLaunchKernelGGL(relax_kernel, dim3(a.B), dim3(NT), bytes, st, a);
    return abx_check_launch("abx_relax");
}
