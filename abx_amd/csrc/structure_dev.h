// The structure conventions of the per-design analyses (design scores, relax, interface, polar contacts, accuracy), in one place.
// Every Abx*Args of these entries begins with the same fields (include/abx_hip.h: pred_atom14 ... gt_seq, then radius, L, Lab), so one
// template reads them all:
//   - rows < Lpred come from the prediction, the rest from the ground truth;
//   - the residue type of a row < Lab is the predicted token, of the others the ground truth's;
//   - tokens outside 0..20 are the unknown type 20;
//   - an atom exists if res_mask keeps its row and then, in this order: pred_mask says so when it is given, the radius table has the
//     slot for a predicted row, gt_exists has it for a ground-truth row.
// Plain C++ only (no builtins, no shuffles): tests compile this header for the host, alone and under relax.hip.
#pragma once
#include <cstdio>

// One structure of the batch as the kernels read it.  `g`: the row offset of this structure's complex (0: one complex for the batch).
template <class Args>
struct StructureView {
    const float* pred; const float* gt;
    const long long* pseq; const long long* gseq;
    const unsigned char* pmask; const unsigned char* gexists; const unsigned char* rmask;
    const float* radius;
    int Lab, Lpred;
    __device__ __forceinline__ StructureView(const Args& a, int b, long long g = 0) {
        pred = a.pred_atom14 + (long long)b * a.pred_sb;
        gt = a.gt_atom14 + g * 42;
        pseq = a.pred_seq + (long long)b * a.pred_seq_sb;
        gseq = a.gt_seq + g;
        pmask = a.pred_mask ? a.pred_mask + (long long)b * a.L * 14 : nullptr;
        gexists = a.gt_exists + g * 14;
        rmask = a.res_mask;
        radius = a.radius;
        Lab = a.Lab; Lpred = a.Lpred;
    }
    static __device__ __forceinline__ int clamp_aa(long long aa) { return aa < 0 ? 20 : (aa > 20 ? 20 : (int)aa); }
    __device__ __forceinline__ int aatype(int res) const {
        const long long aa = res < Lab ? pseq[res] : gseq[res];
        return aa < 0 ? 20 : (aa > 20 ? 20 : (int)aa);
    }
    __device__ __forceinline__ const float* xyz(int res, int slot) const {
        return (res < Lpred ? pred : gt) + ((long long)res * 14 + slot) * 3;
    }
    __device__ __forceinline__ bool kept(int res) const { return !rmask || rmask[res] != 0; }
    __device__ __forceinline__ bool exists(int res, int slot, int aa) const {
        if (rmask && !rmask[res]) return false;
        if (pmask) return pmask[(long long)res * 14 + slot] != 0;
        return res < Lpred ? radius[aa * 14 + slot] > 0.f : gexists[(long long)res * 14 + slot] != 0;
    }
};

// The argument checks that every entry with a StructureView makes before its own: sizes, Lab, Lpred and the operands the view reads.
// `lpred_lab_or_L`: the prediction covers the antibody or the whole complex, nothing between (accuracy).  Returns ABX_OK or ABX_ERR_ARG
// with "<entry>: ..." as the last error (abx_set_error copies the text).
template <class Args>
inline int abx_check_structure_args(const Args& a, const char* entry, int min_L, bool lpred_lab_or_L = false) {
    const char* what = nullptr;
    if (!(a.B > 0 && a.L >= min_L && a.B <= 65535 && a.L < (1 << 22))) what = min_L > 1 ? "bad sizes (B > 0, L > 1)" : "bad sizes";
    else if (!(a.Lab > 0 && a.Lab <= a.L)) what = "Lab must be in 1..L";
    else if (lpred_lab_or_L ? !(a.Lpred == a.Lab || a.Lpred == a.L) : !(a.Lpred >= a.Lab && a.Lpred <= a.L))
        what = lpred_lab_or_L ? "Lpred must be Lab or L" : "Lpred must be in Lab..L";
    else if (!(a.pred_atom14 && a.pred_seq && a.gt_atom14 && a.gt_exists && a.gt_seq && a.radius)) what = "null operand";
    if (!what) return ABX_OK;
    char msg[128];
    snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    abx_set_error(msg);
    return ABX_ERR_ARG;
}
