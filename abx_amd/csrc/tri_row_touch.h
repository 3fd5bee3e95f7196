// Which bytes of a pair row z[b, s, :, :] the row-fused triangle attention (attention.hip tri_attn8_rowfused_kernel) reads, and when.
// Host and device: the kernel computes its addresses with these functions, tests/test_tri_row_touch_host.py checks them on the CPU.
//
// A position l of the row holds 192 fp32 channels = 768 bytes = six 128-byte lines (lines are counted from the position's first channel).
// Phase P walks the row k-group outer: k-group g = k-tiles 4 g .. 4 g + 3 = channels 64 g .. 64 g + 63 = lines 2 g and 2 g + 1 of every
// position; nothing is read twice inside a workgroup.  The issuing wave touches the lines of k-group g (one 4-byte load per line) shortly
// before the computing waves walk them (TriRowArgs.touch == 2), or the whole row a phase ahead (touch == 1).
// All offsets are in floats from z[b, s, 0, 0]; zl is the stride of a position.
#pragma once
#ifndef __host__
#define __host__
#define __device__
#endif

constexpr int RFT_CH = 192;                  // channels of a position
constexpr int RFT_LINE = 32;                 // floats of a 128-byte line
constexpr int RFT_KGROUPS = 3;               // k-groups of the walk
constexpr int RFT_KG_LINES = 2;              // lines of a k-group per position
constexpr int RFT_LANES = 64;                // lanes of the issuing wave: the touch stride over positions
constexpr int RFT_LMAX = 352;                // the longest row the kernel takes
constexpr int RFT_POS = (RFT_LMAX + RFT_LANES - 1) / RFT_LANES;      // positions a lane touches: 6
constexpr int RFT_N = RFT_POS * RFT_KG_LINES;                        // touch loads per k-group: 12 instructions, whatever L is

// ---- the touch: load i (0 .. RFT_N - 1) of lane `lane` for k-group g.  Position lane + 64 (i / 2), line 2 g + (i & 1).
// The number of loads does not depend on L (the issuing wave counts its outstanding vector-memory instructions): a load whose position
// lies beyond the row is not active and goes to the row's last position again.
__host__ __device__ inline bool rf_touch_active(int L, int lane, int i) { return lane + RFT_LANES * (i / RFT_KG_LINES) < L; }
__host__ __device__ inline long long rf_touch_offset(int L, long long zl, int g, int lane, int i) {
    const int l = lane + RFT_LANES * (i / RFT_KG_LINES);
    return (long long)(l < L ? l : L - 1) * zl + (RFT_KG_LINES * g + (i % RFT_KG_LINES)) * RFT_LINE;
}

// ---- the walk: computing wave `wave`, lane (pr = position of the wave's 32, hh = channel half of a k-tile) reads the 8 floats from
// rf_walk_base + rf_walk_ktile(kt) for the k-tiles kt = 4 g .. 4 g + 3 of k-group g.  Positions beyond the row: the last one again.
__host__ __device__ inline int rf_walk_pos(int L, int wave, int pr) { const int l = 32 * wave + pr; return l < L ? l : L - 1; }
__host__ __device__ inline long long rf_walk_base(int L, long long zl, int wave, int pr, int hh) { return (long long)rf_walk_pos(L, wave, pr) * zl + 8 * hh; }
__host__ __device__ constexpr int rf_walk_ktile(int kt) { return kt * 16; }
constexpr int RFT_WALK_FLOATS = 8;           // floats of one walk read (two 16-byte loads)
