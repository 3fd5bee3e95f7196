// Frame pull-back of per-atom gradients, shared by guidance.hip (abx_clash_grad) and contact.hip (abx_contact_grad): with
// x_a = R_i p_a + t_i,   dE/dt_i = sum_a g_a   and   dE/d(rotation vector of R_i, world frame) = sum_a (x_a - t_i) x g_a
// over the existing atoms of residue i, slots in ascending order (fixed summation order).  One thread per residue, strided by `nthreads`.
#pragma once

__device__ __forceinline__ void frame_pullback(const float* atom14, const unsigned char* atom_mask,
                                               const float* grad_atom, const float* frame_trans,
                                               float* grad_trans, float* grad_rot, long long ab, int L, int tid,
                                               int nthreads) {
    for (int i = tid; i < L; i += nthreads) {
        const long long r = ab + i;
        const float* t = frame_trans + r * 3;
        float ft[3] = {0.f, 0.f, 0.f}, tq[3] = {0.f, 0.f, 0.f};
        for (int s = 0; s < 14; ++s) {
            if (!atom_mask[r * 14 + s]) continue;
            const float* x = atom14 + (r * 14 + s) * 3;
            const float* g = grad_atom + (r * 14 + s) * 3;
            const float rx = x[0] - t[0], ry = x[1] - t[1], rz = x[2] - t[2];
            ft[0] += g[0]; ft[1] += g[1]; ft[2] += g[2];
            tq[0] += ry * g[2] - rz * g[1];
            tq[1] += rz * g[0] - rx * g[2];
            tq[2] += rx * g[1] - ry * g[0];
        }
        for (int k = 0; k < 3; ++k) {
            grad_trans[r * 3 + k] = ft[k];
            grad_rot[r * 3 + k] = tq[k];
        }
    }
}
