// cf2sim_hj.h -- HJ value-table lookup: nearest grid node and the disturbance sign bits
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf2sim_internal.h"

namespace cf2 {

// ------------------------------------------------------------------------------------
// HJ value-table gather (7 taps: centre and +-1 along the three rate dims)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ int grid_nearest(const double* pts, double s) {
    // searchsorted(side='left') on the sorted nodes = the number of nodes below s: a branch-free
    // binary search over 16 slots (slot 15 is +inf), 4 compares instead of 15
    static_assert(HJ_PTS == 15, "16-slot search");
    int idx = 0;
#pragma unroll
    for (int step = 8; step >= 1; step >>= 1) {
        const int k = idx + step - 1;
        idx += (k < HJ_PTS && pts[k < HJ_PTS ? k : HJ_PTS - 1] < s) ? step : 0;
    }
    if (idx > 0 && (idx == HJ_PTS || fabs(s - pts[idx - 1]) < fabs(s - pts[idx]))) return idx - 1;
    return idx;
}
__device__ __forceinline__ float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// returns bit i set <=> dV/dx_{3+i} > 0 (opt disturbance = -dmax_i).  grid: the 6 x 15 grid
// points (KTables::hj_grid) staged in LDS by the calling kernel: the nearest-node searches then
// cost LDS round trips instead of serialised global loads.
// distur_gener's sign rule at grid node c (flat index) with per-dim indices idx: for each rate
// dimension d = 3..5 the one-sided differences L, R of V around the node (GridProcessing.py
// spatial derivative with the boundary extrapolation of distur_gener.py:160-183), bit d-3 = L > -R
__device__ __forceinline__ unsigned hj_node_bits(const float* __restrict__ V, int c, const int idx[6]) {
    const int stride[6] = {759375, 50625, 3375, 225, 15, 1};
    const float Vc = V[c];
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int d = 3 + i;
        const int s = stride[d];
        float L, Rr;
        if (idx[d] == 0) {
            const float Vn = V[c + s];
            const float lb = __fadd_rn(Vc, __fmul_rn(fabsf(__fsub_rn(Vn, Vc)), sgnf(Vc)));
            L = __fsub_rn(Vc, lb); Rr = __fsub_rn(Vn, Vc);
        } else if (idx[d] == HJ_PTS - 1) {
            const float Vp = V[c - s];
            const float rb = __fadd_rn(Vc, __fmul_rn(fabsf(__fsub_rn(Vc, Vp)), sgnf(Vc)));
            L = __fsub_rn(Vc, Vp); Rr = __fsub_rn(rb, Vc);
        } else {
            const float Vp = V[c - s], Vn = V[c + s];
            L = __fsub_rn(Vc, Vp); Rr = __fsub_rn(Vn, Vc);
        }
        bits |= (L > -Rr ? 1u : 0u) << i;
    }
    return bits;
}
// nearest grid node of a state (Grid.get_index, GridProcessing.py:52-71): flat index and per-dim indices
__device__ __forceinline__ int hj_node(const double st[6], const double* grid, int idx[6]) {
    const int stride[6] = {759375, 50625, 3375, 225, 15, 1};
    int c = 0;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        idx[d] = grid_nearest(grid + d * HJ_PTS, st[d]);
        c += idx[d] * stride[d];
    }
    return c;
}
__device__ __forceinline__ unsigned hj_signs(const float* __restrict__ V, const double st[6], const double* grid) {
    int idx[6];
    const int c = hj_node(st, grid, idx);
    return hj_node_bits(V, c, idx);
}

// every thread of the block takes part (contains a block barrier)
__device__ __forceinline__ void stage_hj_grid(const double (*src)[HJ_PTS], double* s_grid) {
    for (uint32_t k = threadIdx.x; k < 6u * HJ_PTS; k += blockDim.x) s_grid[k] = src[k / HJ_PTS][k % HJ_PTS];
    __syncthreads();
}

}  // namespace cf2
