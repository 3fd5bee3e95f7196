// The rules about a residue row that developability.hip and patches.hip share: which cdr_def codes are CDRs, the residue-type constants,
// the unit charge of a type, the fixed-point one, and the exposure rule - a row is exposed when the solvent-accessible area of its side
// chain reaches the fraction `exposed` of its type's reference area.  The host twins are abx_amd.developability (CDR_CODES, FIXED_ONE,
// side_chain_area) and abx_amd.patches.
// Plain C++ only (no builtins, no shuffles): a test compiles this header for the host.  Like structure_dev.h it includes nothing: the
// includer brings common.h first (on the host the stand-in of tests/relax_emu), which defines __device__ and __forceinline__.
#pragma once

#pragma clang fp contract(off)

constexpr double FIXED_ONE = 1073741824.0;     // 2^30
// residue types (residue_constants.restypes)
constexpr int T_ARG = 1, T_ASN = 2, T_ASP = 3, T_CYS = 4, T_GLU = 6, T_GLY = 7, T_HIS = 8, T_LYS = 11, T_MET = 12, T_PRO = 14, T_SER = 15,
              T_THR = 16, T_TRP = 17;

__device__ __forceinline__ bool is_cdr(int c) { return c == 1 || c == 3 || c == 5 || c == 8 || c == 10 || c == 12; }

__device__ __forceinline__ int type_charge(int aa) { return (aa == T_LYS || aa == T_ARG ? 1 : 0) - (aa == T_ASP || aa == T_GLU ? 1 : 0); }

// Solvent-accessible area of the side chain of `row` (type aa): over the slots 4..13 in this order, the free points of a counted atom
// (a positive radius, and it exists) times the area of one point.  `pts`: (L,14,2) of the structure, `a`: [21][14].
template <class View>
__device__ __forceinline__ double sidechain_rel_area(const View& s, const float* radius, const int* pts, const double* a, int row, int aa) {
    double rel = 0.0;
    for (int sl = 4; sl < 14; ++sl) {
        const bool counted = radius[aa * 14 + sl] > 0.f && s.exists(row, sl, aa);
        rel = rel + (double)(counted ? pts[2 * (row * 14 + sl)] : 0) * a[aa * 14 + sl];
    }
    return rel;
}

__device__ __forceinline__ bool row_exposed(double rel, double ref, double exposed) { return ref > 0.0 && rel >= exposed * ref; }
