// Device idioms shared by the split-f16 kernels (gemm3_mainloop.h, gemm3.hip, tails.hip, gemm_as.hip, opm.hip, assemble_bias.hip,
// attention.hip).  The plane swizzle (plane_off) and the pair-row map (pair_a_row) are CONTRACTS between kernels, not conveniences: a
// producer GEMM writes images that another file's kernel reads by the same formula, and the bit-identity tests between the A-stationary
// and the tile kernels rest on both taking their A rows through the same map.  One definition of each.
#pragma once
#include <type_traits>

#include "common.h"
#include "abx_hip.h"

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

// 16 bytes per lane, global -> LDS at (wave-uniform) dst + lane * 16
__device__ __forceinline__ void glds16(const void* src, char* dst_wave_base) {
    __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)dst_wave_base, 16, 0, 0);
}

// A per-lane 32-bit byte offset as the compiler must see it AT the DMA instruction: defined in the same basic block, so that the
// address is (scalar base) + zext(32-bit VGPR) and the load takes the scalar-base form `global_load_lds v, s[a:a+1]`.  Hoisted out
// of the k loop the zero-extension becomes a 64-bit VGPR pair and every DMA instruction a v_lshl_add_u64 first (4 VALU instructions
// and 4 VGPRs per k-step of the 128 x 128 tile).
__device__ __forceinline__ unsigned vgpr32(unsigned o) {
    asm volatile("" : "+v"(o));
    return o;
}

// the newest N vector-memory operations of this wave may stay in flight (results return in issue order)
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// byte offset of (plane, row, 16-byte half) in a [2][ROWS][16] 16-bit tile image: the two 16-byte halves swapped on odd row-octets, so
// that 16-byte fragment reads with lane -> row, lane >> 5 -> k half are conflict-free
template <int ROWS> __device__ __forceinline__ int plane_off(int plane, int row, int half) {
    return plane * (ROWS * 32) + row * 32 + ((half ^ ((row >> 3) & 1)) << 4);
}

// compile-time loop: f(IC<I0>{}), ..., f(IC<I1 - 1>{}) - the index is a constant expression inside f
template <int I> using IC = std::integral_constant<int, I>;
template <int I0, int I1, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I0 < I1) {
        f(IC<I0>{});
        static_for<I0 + 1, I1>(f);
    }
}

// 4 x 4 transpose inside every lane quad: lane q of a quad holds x[0 .. 3] = rows 0 .. 3 of column q and receives o[0 .. 3] = columns
// 0 .. 3 of row q.  Two exchange stages (lane ^ 1, lane ^ 2), each ONE v_cndmask_b32 with a DPP quad_perm source per value (the select
// and the cross-lane move in one instruction; vcc = the lanes that keep their own value): 8 VALU instructions instead of the 24 the
// compiler makes of update_dpp + select (a zeroed destination, the move, the select).  The leading s_nop covers the two wait states
// between the VALU write of x and its DPP read; inside the statement every DPP source is written >= 2 instructions earlier.
__device__ __forceinline__ void quad_transpose(const float (&x)[4], float (&o)[4]) {
    float a0, a1, a2, a3;
    asm volatile(
        "s_nop 1\n\t"
        "s_mov_b32 vcc_lo, 0x55555555\n\ts_mov_b32 vcc_hi, 0x55555555\n\t"                                    // even lanes keep rows 0, 2
        "v_cndmask_b32_dpp %4, %9, %8, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"               // a0 = even ? x0 : x1 of lane ^ 1
        "v_cndmask_b32_dpp %6, %11, %10, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"             // a2 = even ? x2 : x3 of lane ^ 1
        "s_mov_b32 vcc_lo, 0xaaaaaaaa\n\ts_mov_b32 vcc_hi, 0xaaaaaaaa\n\t"                                    // odd lanes keep rows 1, 3
        "v_cndmask_b32_dpp %5, %8, %9, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"               // a1 = odd ? x1 : x0 of lane ^ 1
        "v_cndmask_b32_dpp %7, %10, %11, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"             // a3 = odd ? x3 : x2 of lane ^ 1
        "s_mov_b32 vcc_lo, 0x33333333\n\ts_mov_b32 vcc_hi, 0x33333333\n\t"                                    // lanes 0, 1 of a quad
        "v_cndmask_b32_dpp %0, %6, %4, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"               // o0 = low ? a0 : a2 of lane ^ 2
        "v_cndmask_b32_dpp %1, %7, %5, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"               // o1 = low ? a1 : a3 of lane ^ 2
        "s_mov_b32 vcc_lo, 0xcccccccc\n\ts_mov_b32 vcc_hi, 0xcccccccc\n\t"                                    // lanes 2, 3 of a quad
        "v_cndmask_b32_dpp %2, %4, %6, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"               // o2 = high ? a2 : a0 of lane ^ 2
        "v_cndmask_b32_dpp %3, %5, %7, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"                     // o3 = high ? a3 : a1 of lane ^ 2
        : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3)
        : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3])
        : "vcc");
}

// Source row (of the operand's batch entry) of GEMM row gri of a k-contiguous fp32 A: the identity, the pair transposition
// (a_pair_transpose: row (q, r) of an L x L tensor reads row (r, q)), or - a_pair - the padded pair position (i, j) of the GEMM -> row
// of the unpadded pair tensor (pad columns re-read column L - 1; their outputs are zeroed by the row scale / never stored), the GEMM rows
// in row-major or in (8 i x 16 k) block order (c_split_tile: pair_tile_decode).
// (gri is 32-bit: M < 2^31; 64-bit divisions cost ~80 instructions)
__device__ __forceinline__ long long pair_a_row(const AbxGemm& g, int gri) {
    long long gr = gri;
    if (g.a_pair) {
        int pi, pj;
        if (g.c_split_tile) {
            pair_tile_decode(gri, g.pair_Lp, pi, pj);
            pi = min(pi, g.pair_L - 1);
            pj = min(pj, g.pair_L - 1);
        } else {
            pi = gri / g.pair_Lp;
            pj = min(gri - pi * g.pair_Lp, g.pair_L - 1);
        }
        gr = g.a_pair_transpose > 0 ? (long long)pj * g.pair_L + pi : (long long)pi * g.pair_L + pj;
    } else if (g.a_pair_transpose > 0) {
        const int qi = gri / g.a_pair_transpose;
        gr = (long long)(gri - qi * g.a_pair_transpose) * g.a_pair_transpose + qi;
    }
    return gr;
}
