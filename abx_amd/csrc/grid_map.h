// The XCD-contiguous workgroup remap of the 1-D grids.  Host and device: the kernels call it on blockIdx.x,
// tests/test_grid_map_host.py checks its guarantees on the CPU.
//
// Workgroups are placed round-robin over the 8 XCDs (blocks with the same bid & 7 share an XCD and its private L2).  The remap hands
// every XCD a CONTIGUOUS range of the work items: the N-tiles that share an A panel, all tiles of one batch entry of the
// triangle-multiplication contraction, the (b, i) rows of one sample meet in one L2.
// Guarantees, for any nwg >= 1:
//   - bid -> xcd_contiguous(bid, nwg) is a bijection of 0 .. nwg - 1;
//   - the blocks of XCD x (bid & 7 == x), in launch order, take one contiguous ascending range;
//   - the ranges are ordered by x, and their sizes differ by at most one (the first nwg & 7 XCDs hold one item more).
// Placement is a performance matter only: no kernel's result depends on it.
// (32-bit: the dispatchers keep the grids below 2^31 items; a 64-bit division is ~80 instructions in front of a block's first DMA)
#pragma once
#ifndef __host__
#define __host__
#define __device__
#endif

__host__ __device__ inline unsigned xcd_contiguous(unsigned bid, unsigned nwg) {
    const unsigned q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}
