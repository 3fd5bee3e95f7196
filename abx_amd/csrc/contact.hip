// Interface guidance terms (BASELINE north_star "the evolutionary/physical/geometric guidance-gradient terms", "guidance
// pairwise-distance/clash terms"): the geometric half beside the violation terms of guidance.hip.  No reference site (the reference
// samples without guidance); the constants come from the interface table (4 A heavy-atom contacts) and upstream's
// 8 A pseudo-beta contacts.  Energies and conventions: include/abx_hip.h, AbxContactArgs.
//
// Three kernels, no atomics, every sum in a fixed order, nothing shared between the samples of a batch:
//   hotspot_stats_kernel   one wave per (sample, hotspot): lanes walk the moved rows, max and sum of exp(-beta d) through wave
//                          shuffles; m_h, the log-normaliser, w_hot Hub'(m_h - d_hot) and the hotspot's energy go to the workspace
//   contact_kernel         the shape of clash_kernel: a block owns 16 residues (224 atoms, one thread each) and leaves by a uniform
//                          branch when none of them is moved; the partner atoms stream through a 16-residue float4 LDS tile (tiles
//                          without a partner atom are skipped by a uniform branch); the thread accumulates the force on ITS atom:
//                          contacts, the hotspot term if it is a pseudo-beta (softmax weight x Hub' x unit vector), and the restraints
//                          that name its (row, slot), found by scanning the table in LDS (a gather: no two threads write one atom)
//   contact_frames_kernel  restraint energies (one thread each), the fixed-order energy sums, the frame pull-back of frame_dev.h
#include "common.h"
#include "abx_hip.h"
#include "frame_dev.h"

namespace {

constexpr int RT = 16;                 // residues per tile
constexpr int AT = RT * 14;            // atoms per tile (224)
constexpr int MAXH = 64;               // hotspots
constexpr int MAXR = 256;              // restraints
constexpr int HS = 4;                  // workspace floats per (sample, hotspot): m_h, log-normaliser, w_hot Hub'(m_h - d_hot), energy

__device__ __forceinline__ float dist3(float dx, float dy, float dz) { return sqrtf(1e-10f + dx * dx + dy * dy + dz * dz); }
__device__ __forceinline__ float hub(float v) { return v <= 0.f ? 0.f : (v < 1.f ? 0.5f * v * v : v - 0.5f); }
__device__ __forceinline__ float hub_d(float v) { return v <= 0.f ? 0.f : (v < 1.f ? v : 1.f); }
// atom14 slot of the pseudo-beta of a row (CB, else CA), -1: none
__device__ __forceinline__ int pb_slot(const unsigned char* m) { return m[4] ? 4 : (m[1] ? 1 : -1); }
// (row << 4 | slot) of a restraint end, -1 when it is out of range
__device__ __forceinline__ int restraint_key(int row, int slot, int L) {
    return (row >= 0 && row < L && slot >= 0 && slot < 14) ? (row << 4) | slot : -1;
}

__global__ __launch_bounds__(64) void hotspot_stats_kernel(const AbxContactArgs a, float* __restrict__ hs) {
    const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x, L = a.L;
    const long long ab = (long long)b * L;
    float* o = hs + ((long long)b * a.H + k) * HS;
    const int h = a.hotspots[k];
    int hsl = -1;
    if (h >= 0 && h < L && !a.moved[ab + h]) hsl = pb_slot(a.atom_mask + (ab + h) * 14);
    float hx = 0.f, hy = 0.f, hz = 0.f;
    if (hsl >= 0) {
        const float* p = a.atom14 + ((ab + h) * 14 + hsl) * 3;
        hx = p[0]; hy = p[1]; hz = p[2];
    }
    // v_i = -beta d_i of the moved rows with a pseudo-beta: the maximum first, then the sum with the maximum subtracted
    float mx = ABX_NEG_MAX;
    if (hsl >= 0) {
        for (int i = lane; i < L; i += 64) {
            if (!a.moved[ab + i]) continue;
            const int s = pb_slot(a.atom_mask + (ab + i) * 14);
            if (s < 0) continue;
            const float* p = a.atom14 + ((ab + i) * 14 + s) * 3;
            mx = fmaxf(mx, -a.beta * dist3(p[0] - hx, p[1] - hy, p[2] - hz));
        }
    }
    mx = wave_max(mx);
    if (mx == ABX_NEG_MAX) {                                  // uniform: inactive hotspot, or no moved pseudo-beta in this sample
        if (lane < HS) o[lane] = 0.f;
        return;
    }
    float sum = 0.f;
    for (int i = lane; i < L; i += 64) {
        if (!a.moved[ab + i]) continue;
        const int s = pb_slot(a.atom_mask + (ab + i) * 14);
        if (s < 0) continue;
        const float* p = a.atom14 + ((ab + i) * 14 + s) * 3;
        sum += expf(-a.beta * dist3(p[0] - hx, p[1] - hy, p[2] - hz) - mx);
    }
    sum = wave_sum(sum);
    if (lane == 0) {
        const float c = mx + logf(sum), m = -c / a.beta, v = m - a.d_hot;
        o[0] = m;
        o[1] = c;
        o[2] = a.w_hot * hub_d(v);
        o[3] = a.w_hot * hub(v);
    }
}

__global__ __launch_bounds__(256) void contact_kernel(const AbxContactArgs a, const float* __restrict__ hs, float* __restrict__ epart) {
    __shared__ float4 tile[AT];        // x, y, z, w > 0: an existing atom of a target row that is not moved
    __shared__ float4 hpos[MAXH];      // pseudo-beta of the hotspot, w = w_hot Hub'(m_h - d_hot) (0: nothing to add)
    __shared__ float hnorm[MAXH];      // log-normaliser of the hotspot's soft minimum
    __shared__ int rkey[MAXR][2];      // restraint ends as (row << 4 | slot), -1: out of range
    __shared__ float rpar[MAXR][3];    // lo, hi, weight
    __shared__ float ered[4];
    const int b = blockIdx.y, it = blockIdx.x, tid = threadIdx.x, L = a.L;
    const long long ab = (long long)b * L;
    const int mres = it * RT + tid / 14, mslot = tid % 14;
    const bool mine = tid < AT && mres < L;
    const bool mv = mine && a.moved[ab + mres] != 0;
    float* gout = a.grad_atom + ((ab + (mine ? mres : 0)) * 14 + mslot) * 3;
    if (!__syncthreads_or(mv ? 1 : 0)) {                      // uniform: no moved row in this block
        if (mine) { gout[0] = 0.f; gout[1] = 0.f; gout[2] = 0.f; }
        if (tid == 0) epart[(long long)b * gridDim.x + it] = 0.f;
        return;
    }
    for (int k = tid; k < a.H; k += 256) {
        const float* s = hs + ((long long)b * a.H + k) * HS;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        const int h = a.hotspots[k];
        if (s[2] != 0.f && h >= 0 && h < L) {                 // (an active hotspot has a pseudo-beta: hotspot_stats_kernel)
            const int sl = pb_slot(a.atom_mask + (ab + h) * 14);
            if (sl >= 0) {
                const float* x = a.atom14 + ((ab + h) * 14 + sl) * 3;
                p = make_float4(x[0], x[1], x[2], s[2]);
            }
        }
        hpos[k] = p;
        hnorm[k] = s[1];
    }
    for (int r = tid; r < a.R; r += 256) {
        const int* q = a.restr_idx + r * 4;
        const int ki = restraint_key(q[0], q[1], L), kj = restraint_key(q[2], q[3], L);
        const bool ok = ki >= 0 && kj >= 0 && ki != kj;
        rkey[r][0] = ok ? ki : -1;
        rkey[r][1] = ok ? kj : -1;
        rpar[r][0] = a.restr_par[r * 3];
        rpar[r][1] = a.restr_par[r * 3 + 1];
        rpar[r][2] = a.restr_par[r * 3 + 2];
    }
    // my atom: forces act on existing atoms of moved rows only
    float mx = 0.f, my = 0.f, mz = 0.f;
    bool act = false, is_pb = false;
    if (mv) {
        const unsigned char* mk = a.atom_mask + (ab + mres) * 14;
        act = mk[mslot] != 0;
        is_pb = act && pb_slot(mk) == mslot;
        const float* x = a.atom14 + ((ab + mres) * 14 + mslot) * 3;
        mx = x[0]; my = x[1]; mz = x[2];
    }
    float gx = 0.f, gy = 0.f, gz = 0.f, ssum = 0.f;
    const float inv = 1.0f / (a.d1 - a.d0);
    const bool contacts = a.w_contact != 0.f;                 // uniform
    for (int jt = 0; contacts && jt < (L + RT - 1) / RT; ++jt) {
        __syncthreads();
        int ok = 0;
        if (tid < AT) {
            const int res = jt * RT + tid / 14;
            float4 p = make_float4(0.f, 0.f, 0.f, -1.f);
            if (res < L) {
                const long long r = ab + res;
                ok = (a.target[res] != 0 && a.moved[r] == 0 && a.atom_mask[r * 14 + tid % 14] != 0) ? 1 : 0;
                const float* x = a.atom14 + (r * 14 + tid % 14) * 3;
                p = make_float4(x[0], x[1], x[2], ok ? 1.f : -1.f);
            }
            tile[tid] = p;
        }
        if (!__syncthreads_or(ok)) continue;                  // uniform: no partner atom in this tile
        if (act) {
            for (int k = 0; k < AT; ++k) {
                const float4 o = tile[k];
                if (o.w <= 0.f) continue;
                const float dx = mx - o.x, dy = my - o.y, dz = mz - o.z;
                const float d = dist3(dx, dy, dz);
                if (d >= a.d1) continue;
                if (d <= a.d0) { ssum += 1.0f; continue; }
                const float u = (d - a.d0) * inv, t = 1.0f - u * u;
                ssum += t * t;
                const float s = a.w_contact * 4.0f * u * t * inv / d;      // -w ds/dd / d,  ds/dd = -4 u (1 - u^2) / (d1 - d0)
                gx += s * dx; gy += s * dy; gz += s * dz;
            }
        }
    }
    __syncthreads();                                          // hpos / rkey are written (no tile loop without the contact term)
    if (is_pb) {
        for (int k = 0; k < a.H; ++k) {
            const float4 hp = hpos[k];
            if (hp.w == 0.f) continue;
            const float dx = mx - hp.x, dy = my - hp.y, dz = mz - hp.z;
            const float d = dist3(dx, dy, dz);
            const float s = hp.w * expf(-a.beta * d - hnorm[k]) / d;       // w_hot Hub' x softmax weight x unit vector
            gx += s * dx; gy += s * dy; gz += s * dz;
        }
    }
    if (act) {
        const int key = (mres << 4) | mslot;
        for (int r = 0; r < a.R; ++r) {
            const int ki = rkey[r][0], kj = rkey[r][1];
            const int other = ki == key ? kj : (kj == key ? ki : -1);
            if (other < 0) continue;
            const long long oa = (ab + (other >> 4)) * 14 + (other & 15);
            if (!a.atom_mask[oa]) continue;
            const float* x = a.atom14 + oa * 3;
            const float dx = mx - x[0], dy = my - x[1], dz = mz - x[2];
            const float d = dist3(dx, dy, dz);
            const float s = rpar[r][2] * (hub_d(d - rpar[r][1]) - hub_d(rpar[r][0] - d)) / d;
            gx += s * dx; gy += s * dy; gz += s * dz;
        }
    }
    if (mine) { gout[0] = gx; gout[1] = gy; gout[2] = gz; }
    float e = wave_sum(-a.w_contact * ssum);
    if ((tid & 63) == 0) ered[tid >> 6] = e;
    __syncthreads();
    if (tid == 0) epart[(long long)b * gridDim.x + it] = (ered[0] + ered[1]) + (ered[2] + ered[3]);
}

__global__ __launch_bounds__(256) void contact_frames_kernel(const AbxContactArgs a, const float* __restrict__ hs,
                                                             const float* __restrict__ epart, int nparts) {
    __shared__ float esh[MAXR];
    const int b = blockIdx.x, tid = threadIdx.x, L = a.L;
    const long long ab = (long long)b * L;
    float er = 0.f;
    if (tid < a.R) {
        const int* q = a.restr_idx + tid * 4;
        const int ki = restraint_key(q[0], q[1], L), kj = restraint_key(q[2], q[3], L);
        if (ki >= 0 && kj >= 0 && ki != kj) {
            const long long ia = (ab + (ki >> 4)) * 14 + (ki & 15), ja = (ab + (kj >> 4)) * 14 + (kj & 15);
            if (a.atom_mask[ia] && a.atom_mask[ja]) {
                const float* x = a.atom14 + ia * 3;
                const float* y = a.atom14 + ja * 3;
                const float d = dist3(x[0] - y[0], x[1] - y[1], x[2] - y[2]);
                er = a.restr_par[tid * 3 + 2] * (hub(d - a.restr_par[tid * 3 + 1]) + hub(a.restr_par[tid * 3] - d));
            }
        }
    }
    esh[tid] = er;
    __syncthreads();
    if (tid == 0) {
        float ec = 0.f, eh = 0.f, sr = 0.f;
        for (int k = 0; k < nparts; ++k) ec += epart[(long long)b * nparts + k];
        for (int k = 0; k < a.H; ++k) eh += hs[((long long)b * a.H + k) * HS + 3];
        for (int k = 0; k < a.R; ++k) sr += esh[k];
        a.energy[3 * b] = ec;
        a.energy[3 * b + 1] = eh;
        a.energy[3 * b + 2] = sr;
    }
    frame_pullback(a.atom14, a.atom_mask, a.grad_atom, a.frame_trans, a.grad_trans, a.grad_rot, ab, L, tid, 256);
}

}  // namespace

extern "C" long long abx_contact_grad_workspace_bytes(int B, int L, int H) {
    if (B <= 0 || L <= 0 || H < 0) return 0;
    return ((long long)B * H * HS + (long long)B * ((L + RT - 1) / RT)) * sizeof(float);
}

extern "C" int abx_contact_grad(const AbxContactArgs* ap, void* workspace, hipStream_t st) {
    ABX_REQUIRE(ap != nullptr, "abx_contact_grad: null");
    const AbxContactArgs a = *ap;
    ABX_REQUIRE(a.atom14 && a.atom_mask && a.moved && a.target && a.frame_trans && a.energy && a.grad_atom && a.grad_trans && a.grad_rot &&
                    workspace, "abx_contact_grad: null operand");
    ABX_REQUIRE(a.B > 0 && a.L > 1 && a.B <= 65535 && a.L < (1 << 22), "abx_contact_grad: bad sizes");
    ABX_REQUIRE(a.d0 >= 0.f && a.d0 < a.d1 && a.d1 < 1e30f, "abx_contact_grad: the contact range needs 0 <= d0 < d1");
    ABX_REQUIRE(a.beta > 0.f && a.beta < 1e30f, "abx_contact_grad: beta must be positive");
    ABX_REQUIRE(a.H >= 0 && a.H <= MAXH, "abx_contact_grad: at most 64 hotspots");
    ABX_REQUIRE(a.R >= 0 && a.R <= MAXR, "abx_contact_grad: at most 256 restraints");
    ABX_REQUIRE(a.H == 0 || (a.hotspots && a.hotspots_host), "abx_contact_grad: null hotspot table");
    ABX_REQUIRE(a.R == 0 || (a.restr_idx && a.restr_idx_host && a.restr_par && a.restr_par_host), "abx_contact_grad: null restraint table");
    for (int k = 0; k < a.H; ++k)
        ABX_REQUIRE(a.hotspots_host[k] >= 0 && a.hotspots_host[k] < a.L, "abx_contact_grad: hotspot row out of range");
    for (int r = 0; r < a.R; ++r) {
        const int* q = a.restr_idx_host + r * 4;
        ABX_REQUIRE(q[0] >= 0 && q[0] < a.L && q[2] >= 0 && q[2] < a.L, "abx_contact_grad: restraint row out of range");
        ABX_REQUIRE(q[1] >= 0 && q[1] < 14 && q[3] >= 0 && q[3] < 14, "abx_contact_grad: restraint slot out of range");
        ABX_REQUIRE(q[0] != q[2] || q[1] != q[3], "abx_contact_grad: a restraint names one atom twice");
        ABX_REQUIRE(a.restr_par_host[r * 3] <= a.restr_par_host[r * 3 + 1], "abx_contact_grad: restraint needs lo <= hi");
    }
    const int nparts = (a.L + RT - 1) / RT;
    float* hs = reinterpret_cast<float*>(workspace);
    float* epart = hs + (long long)a.B * a.H * HS;
    if (a.H > 0) {
        hipLaunchKernelGGL(hotspot_stats_kernel, dim3(a.H, a.B), dim3(64), 0, st, a, hs);
        int rc = abx_check_launch("abx_contact_grad(hotspots)");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(contact_kernel, dim3(nparts, a.B), dim3(256), 0, st, a, hs, epart);
    int rc = abx_check_launch("abx_contact_grad");
    if (rc) return rc;
    hipLaunchKernelGGL(contact_frames_kernel, dim3(a.B), dim3(256), 0, st, a, hs, epart, nparts);
    return abx_check_launch("abx_contact_grad(frames)");
}
