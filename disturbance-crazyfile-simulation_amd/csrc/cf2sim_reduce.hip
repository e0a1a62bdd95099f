// cf2sim_reduce.hip -- the second level of the update's reductions, across ranks (no env-step code
// here).  A data-parallel update runs every gradient, evaluation and Fisher-vector call as
//
//     rank partial   cf2_ppo_*_partial (cf2sim_ppo.hip): the rank's block partials summed in
//                    block-index order in fp64, not divided, not rounded: P doubles
//     all-gather     every rank receives the blocks of all ranks, [world][P], in rank order
//     reduce         cf2_ppo_reduce (here): the blocks summed in rank order in fp64, divided by the
//                    sum of the ranks' row counts, rounded once
//
// so every rank computes the same words from the same bits in the same order and the weights stay
// in lock step with no broadcast.  world == 1 is ppo_merge_kernel's arithmetic exactly: 0.0 + x is x,
// then the one division by (double)m and the one rounding.  The batch moments (advantages, returns,
// observations) take the same route: {count, mean[D], M2[D]} per rank, folded left in rank order
// with the update of Chan et al. that column_moments_finalize_kernel uses for its block partials.
//
// The TU is compiled with -ffp-contract=off: the written formula is the arithmetic.  No atomics;
// the geometry depends on the sizes only, so the same input gives the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cf2sim.h"
#include "cf2sim_internal.h"
#include "cf2sim_policy.h"

namespace cf2 {

constexpr uint32_t RED_SUM = 8;                // doubles of a block's head: m and the summary slots
constexpr uint32_t RED_MAX_D = 64;             // cf2_column_moments' widest matrix

// blocks [world][P] -> grad[0 .. npar) (already offset to the slice; nullptr: the summary only) and
// summary[0 .. 8).  Every thread sums the row counts itself, in rank order: the same bits everywhere.
// A total of 0 rows: nothing is written.  gate: a non-zero word makes the launch return at once.
__global__ void __launch_bounds__(256) ppo_reduce_kernel(const double* __restrict__ blocks, uint32_t world, uint32_t P,
                                                         uint32_t npar, float* __restrict__ grad,
                                                         double* __restrict__ summary,
                                                         const uint32_t* __restrict__ gate) {
    if (gate && *gate != 0u) return;
    double m = 0.0;
    for (uint32_t r = 0; r < world; ++r) m += blocks[(size_t)r * P];
    if (!(m > 0.0)) return;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (grad && p < npar) {
        double acc = 0.0;
        for (uint32_t r = 0; r < world; ++r) acc += blocks[(size_t)r * P + RED_SUM + p];
        grad[p] = (float)(acc / m);
    }
    if (blockIdx.x == 0 && threadIdx.x < RED_SUM) {
        const uint32_t k = threadIdx.x;
        double acc = 0.0;
        for (uint32_t r = 0; r < world; ++r) acc += blocks[(size_t)r * P + k];
        summary[k] = k == 0 ? m : acc / m;
    }
}

// blocks [world][1 + 2 D] = {count, mean[D], M2[D]} -> out, the same layout; thread d folds column d
// left in rank order.  A block of count 0 is skipped; the first one that counts is taken as it
// stands, so world == 1 returns its input bit for bit.
__global__ void __launch_bounds__(RED_MAX_D) moments_combine_kernel(const double* __restrict__ blocks, uint32_t world,
                                                                    uint32_t D, double* __restrict__ out) {
    const uint32_t d = threadIdx.x, S = 1u + 2u * D;
    if (d >= D) return;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (uint32_t r = 0; r < world; ++r) {
        const double* b = blocks + (size_t)r * S;
        const double bn = b[0], bmean = b[1 + d], bm2 = b[1 + D + d];
        if (!(bn > 0.0)) continue;
        if (n == 0.0) {
            n = bn;
            mean = bmean;
            m2 = bm2;
            continue;
        }
        const double nab = n + bn, delta = bmean - mean;
        mean = mean + delta * (bn / nab);
        m2 = m2 + bm2 + delta * delta * (n * bn / nab);
        n = nab;
    }
    if (d == 0) out[0] = n;
    out[1 + d] = mean;
    out[1 + D + d] = m2;
}

// the head of a rank's moments block: the count; rows == 0 zeroes the means and M2 too
__global__ void __launch_bounds__(2 * RED_MAX_D) moments_head_kernel(double* __restrict__ block, double rows, uint32_t D) {
    const uint32_t t = threadIdx.x;
    if (t == 0) block[0] = rows;
    if (rows == 0.0 && t < 2u * D) block[1 + t] = 0.0;
}

static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

template <int D>
static int reduce_launch(const double* blocks, uint32_t world, int value, float* grad, double* summary,
                         const uint32_t* gate, hipStream_t s) {
    using L = PolicyLayout<D>;
    constexpr uint32_t NPAR_PI = L::P_LOGSTD - L::P_W1, NPAR_V = L::O_MEAN - L::V_W1, P = RED_SUM + NPAR_V;
    static_assert(NPAR_V >= NPAR_PI, "a block is sized for the larger slice");
    const uint32_t npar = value ? NPAR_V : NPAR_PI;
    float* dst = grad ? grad + (value ? L::V_W1 : L::P_W1) : nullptr;
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3(grad ? (npar + 255u) / 256u : 1u), dim3(256), 0, s, blocks, world, P, npar,
                       dst, summary, gate);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}

}  // namespace cf2

using namespace cf2;

extern "C" int cf2_ppo_reduce(const double* blocks_dev, uint32_t world, uint32_t obs_dim, int value, float* grad_dev,
                              double* summary_dev, const uint32_t* ctrl_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (!blocks_dev || !summary_dev || world == 0 || misaligned(blocks_dev, 8) || misaligned(summary_dev, 8) ||
        misaligned(grad_dev, 4) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? reduce_launch<34>(blocks_dev, world, value, grad_dev, summary_dev, ctrl_dev, s)
                         : reduce_launch<42>(blocks_dev, world, value, grad_dev, summary_dev, ctrl_dev, s);
}

extern "C" int cf2_column_moments_partial(const float* x_dev, uint64_t rows, uint32_t D, double* block_dev,
                                          void* scratch_dev, void* stream) {
    if (D == 0 || D > RED_MAX_D || !block_dev || misaligned(block_dev, 8)) return CF2_ERR_INVALID_ARG;
    if (rows != 0 && (!x_dev || !scratch_dev || misaligned(x_dev, 4) || rows > (UINT64_MAX >> 8) / D))
        return CF2_ERR_INVALID_ARG;
    hipLaunchKernelGGL(moments_head_kernel, dim3(1), dim3(2 * RED_MAX_D), 0, (hipStream_t)stream, block_dev, (double)rows, D);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    return cf2_column_moments(x_dev, rows, D, block_dev + 1, scratch_dev, stream);
}

extern "C" int cf2_moments_combine(const double* blocks_dev, uint32_t world, uint32_t D, double* out_dev, void* stream) {
    if (D == 0 || D > RED_MAX_D || !blocks_dev || !out_dev || world == 0 || misaligned(blocks_dev, 8) ||
        misaligned(out_dev, 8))
        return CF2_ERR_INVALID_ARG;
    hipLaunchKernelGGL(moments_combine_kernel, dim3(1), dim3(RED_MAX_D), 0, (hipStream_t)stream, blocks_dev, world, D, out_dev);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}
