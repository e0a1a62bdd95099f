// cf2sim_hjsolve.hip -- Hamilton-Jacobi reachability solver for the HJ value tables (no env-step
// code here): the attitude / body-rate model of include/cf2sim.h (cf2_hj_model) on a 6-D grid,
// first-order per-node Lax-Friedrichs in space, forward Euler in time, fp64 throughout.
//
// One thread per node; a block of 256 consecutive nodes of one (contiguous) rate cube, so the three
// angle indices are block-uniform.  One launch per time step, ping-pong between two buffers; nothing
// is read back by the host between launches.  Per node, in exactly this order (the TU is compiled with
// -ffp-contract=off, so tests/hj_solve_reference.py, NumPy in the same order, gives the same bits):
//
//   for d in 0..5:  Wm, Wp = neighbours along d
//       periodic d: wrap;  else at index 0:    Wm = W + |Wp - W| sgn(W)
//                               at index n-1:  Wp = W + |W - Wm| sgn(W)     (sgn(0) = 0: hj_node_bits' rule)
//       dm = (W - Wm) inv_dx[d];  dp = (Wp - W) inv_dx[d];  a = 0.5 (dm + dp);  e = 0.5 (dp - dm)
//   f0 = p + (q sin(phi) + r cos(phi)) tan(theta)
//   f1 = q cos(phi) - r sin(phi)
//   f2 = (q sin(phi) + r cos(phi)) sec(theta)
//   H = 0;  for d in 0..2:  H += f_d a_d;  H += |f_d| e_d
//           for d in 3..5:  g = c_d (product of the two other rates)
//                           H += g a_d;  H += b_d |a_d|;  H += (|g| + B_d) e_d
//   W' = W + dt (tube ? min(H, 0) : H)
//
// The trigonometric and node-value tables, inv_dx, c, b and B come from the host in fp64
// (cf2sim_api.cpp); the kernel has no division and no libm call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cf2sim.h"
#include "cf2sim_internal.h"

namespace cf2 {

constexpr int HJS_BLOCK = 256, HJS_WAVES = HJS_BLOCK / 64;

__device__ __forceinline__ double sgnd(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

template <bool CHANGE>
__global__ void __launch_bounds__(HJS_BLOCK) hj_solve_step_kernel(const HjSolveArgs A) {
    // the rate nodes are looked up per lane: LDS; the angle tables are read at block-uniform indices
    __shared__ double s_rate[3 * HJS_MAX_PTS];
    __shared__ double s_max[HJS_WAVES];
    for (uint32_t k = threadIdx.x; k < 3u * HJS_MAX_PTS; k += HJS_BLOCK)
        s_rate[k] = A.tab[HJS_RATE_P + k / HJS_MAX_PTS][k % HJS_MAX_PTS];
    __syncthreads();
    // A block works inside one rate cube: its three angle indices are uniform (blockIdx.z = i0 n1 + i1,
    // blockIdx.y = i2), so the angle dimensions' neighbour offsets, boundary cases and trigonometric
    // factors cost scalar instructions, and only the two rate divisions are per lane.  Divisions by
    // a node count n <= HJS_MAX_PTS are __umulhi(x, ceil(2^32 / n)), exact for x n < 2^32 (here
    // x < HJS_MAX_PTS^3).
    const uint32_t c = blockIdx.x * (uint32_t)HJS_BLOCK + threadIdx.x;      // within the rate cube
    double change = 0.0;
    if (c < A.cube) {
        uint32_t idx[6];
        idx[0] = __umulhi(blockIdx.z, A.magic[1]);
        idx[1] = blockIdx.z - idx[0] * A.n[1];
        idx[2] = blockIdx.y;
        const uint32_t c34 = __umulhi(c, A.magic[5]);
        idx[5] = c - c34 * A.n[5];
        idx[3] = __umulhi(c34, A.magic[4]);
        idx[4] = c34 - idx[3] * A.n[4];
        const uint32_t i = (blockIdx.z * A.n[2] + blockIdx.y) * A.cube + c;

        const double W = A.src[i];
        const double sg = sgnd(W);
        double a[6], e[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            const uint32_t s = A.stride[d], last = A.n[d] - 1u;
            const bool periodic = (A.periodic_mask >> d) & 1u;
            const bool lo = idx[d] == 0u, hi = idx[d] == last;
            // a wrapped neighbour on a periodic dimension; the node itself (always in bounds) where a
            // boundary node has no neighbour and extrapolates instead
            const uint32_t im = !lo ? i - s : (periodic ? i + last * s : i);
            const uint32_t ip = !hi ? i + s : (periodic ? i - last * s : i);
            double Wm = A.src[im], Wp = A.src[ip];
            if (!periodic && lo) Wm = W + fabs(Wp - W) * sg;
            if (!periodic && hi) Wp = W + fabs(W - Wm) * sg;
            const double dm = (W - Wm) * A.inv_dx[d], dp = (Wp - W) * A.inv_dx[d];
            a[d] = 0.5 * (dm + dp);
            e[d] = 0.5 * (dp - dm);
        }
        const double sphi = A.tab[HJS_SIN_PHI][idx[0]], cphi = A.tab[HJS_COS_PHI][idx[0]];
        const double tth = A.tab[HJS_TAN_THETA][idx[1]], scth = A.tab[HJS_SEC_THETA][idx[1]];
        const double p = s_rate[idx[3]], q = s_rate[HJS_MAX_PTS + idx[4]], r = s_rate[2 * HJS_MAX_PTS + idx[5]];
        const double mix = q * sphi + r * cphi;
        const double f[3] = {p + mix * tth, q * cphi - r * sphi, mix * scth};
        const double g[3] = {A.c[0] * (q * r), A.c[1] * (p * r), A.c[2] * (p * q)};
        double H = 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            H += f[d] * a[d];
            H += fabs(f[d]) * e[d];
        }
#pragma unroll
        for (int d = 3; d < 6; ++d) {
            H += g[d - 3] * a[d];
            H += A.b[d - 3] * fabs(a[d]);
            H += (fabs(g[d - 3]) + A.B[d - 3]) * e[d];
        }
        const double rate = A.tube ? (H < 0.0 ? H : 0.0) : H;
        const double Wn = W + A.dt * rate;
        A.dst[i] = Wn;
        change = fabs(Wn - W);
    }
    if (CHANGE) {
        // max |W' - W|: non-negative doubles order like their bit patterns, so an unsigned 64-bit
        // maximum is exact and independent of the order of the atomics
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_xor(change, d);
            change = o > change ? o : change;
        }
        if ((threadIdx.x & 63u) == 0u) s_max[threadIdx.x >> 6] = change;
        __syncthreads();
        if (threadIdx.x == 0) {
            double m = s_max[0];
#pragma unroll
            for (int w = 1; w < HJS_WAVES; ++w) m = s_max[w] > m ? s_max[w] : m;
            atomicMax(A.change, (unsigned long long)__double_as_longlong(m));
        }
    }
}

__global__ void __launch_bounds__(HJS_BLOCK) hj_solve_cast_kernel(const double* __restrict__ w, float* __restrict__ out,
                                                                  uint32_t total) {
    const uint32_t i = blockIdx.x * (uint32_t)HJS_BLOCK + threadIdx.x;
    if (i < total) out[i] = (float)w[i];     // round to nearest
}

hipError_t launch_hj_solve(HjSolveArgs A, double* w, double* tmp, uint32_t steps, double dt, double dt_last,
                           float* table_out, double* change, hipStream_t s) {
    // step kernel: x = 256-node chunks of a rate cube, y = i2, z = i0 n1 + i1 (n <= HJS_MAX_PTS keeps
    // y and z far below the 65 535 limit); cast kernel: flat
    const dim3 block(HJS_BLOCK), flat((A.total + HJS_BLOCK - 1u) / HJS_BLOCK);
    const dim3 grid((A.cube + HJS_BLOCK - 1u) / HJS_BLOCK, A.n[2], A.n[0] * A.n[1]);
    A.change = (unsigned long long*)change;
    if (change) {
        const hipError_t e = hipMemsetAsync(change, 0, sizeof(double), s);
        if (e != hipSuccess) return e;
    }
    double* src = w;
    double* dst = tmp;
    for (uint32_t k = 0; k < steps; ++k) {
        const bool last = k + 1u == steps;
        A.src = src;
        A.dst = dst;
        A.dt = last ? dt_last : dt;
        if (last && change) hipLaunchKernelGGL(hj_solve_step_kernel<true>, grid, block, 0, s, A);
        else hipLaunchKernelGGL(hj_solve_step_kernel<false>, grid, block, 0, s, A);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        double* t = src;
        src = dst;
        dst = t;
    }
    if (src != w) {     // an odd number of steps ended in tmp
        const hipError_t e = hipMemcpyAsync(w, src, (size_t)A.total * sizeof(double), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    if (table_out) {
        hipLaunchKernelGGL(hj_solve_cast_kernel, flat, block, 0, s, w, table_out, A.total);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace cf2
