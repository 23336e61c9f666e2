// kernels_tile.h -- what the dense tile sums share (lj_lrc_kernel, disp_tile_kernel, disp_lrc_kernel, rdc_tile_kernel,
// at_triple_kernel).  A tile's partial is a function of its two blocks' atoms (and the box) only, every tile is redone by
// exactly one workgroup, and the sums below run in an order that does not depend on the pass: an incremental pass over the
// moved atoms' blocks leaves the bits of a from-scratch pass ("Tile passes").
#pragma once
#include "device_common.h"

namespace mpmc {

// The tile (I, J) of workgroup (blockIdx.x, blockIdx.y); false: the workgroup has nothing to do and returns.
//   Full pass (sel.n == 0): grid = (ntile [J], ntile [I]).  Tiles are kept for I <= J only; a workgroup with J < I is handed
//   its own slot all the same and clears it (the row sum runs over all ntile * ntile slots).
//   Incremental pass: grid = (ntile, sel.n); workgroup (x, y) redoes the tile of the blocks {sel.blk[y], x}, I <= J.  The
//   tile of two dirty blocks would be met twice, from either entry: it belongs to the EARLIER entry of sel, whatever the
//   two block indices are, and the later entry's workgroup returns.  sel holds each block once, so every tile with a dirty
//   block is redone exactly once and no slot has two writers.
__device__ __forceinline__ bool owned_tile(const DirtyBlocks &sel, int &I, int &J) {
    I = blockIdx.y;
    J = blockIdx.x;
    if (sel.n > 0) {
        const int d = sel.blk[blockIdx.y], o = blockIdx.x;
        for (int k = 0; k < (int)blockIdx.y; ++k)
            if (sel.blk[k] == o) return false;
        I = min(d, o);
        J = max(d, o);
    }
    return true;
}

// pair (i < j) of two real atoms, not frozen-frozen (lj.c:193, coulombic.c:165, disp_expansion.c:7)
__device__ __forceinline__ bool pair_in_sum(int i, int j, int fli, int flj) {
    return (j > i) && (fli & kValid) && (flj & kValid) && !((fli & kFrozen) && (flj & kFrozen));
}

// Sum of `acc` over the W waves of the workgroup -> out[0]: the butterfly inside a wave, then the waves left to right.
// red: W doubles of LDS.  Every thread of the workgroup calls it.
template <int W>
__device__ __forceinline__ void block_sum_store(double acc, double *red, double *__restrict__ out) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {  // waves in order: deterministic
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < W; ++k) t += red[k];
        out[0] = t;
    }
}

}  // namespace mpmc
