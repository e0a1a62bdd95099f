// cf2sim_optim.hip -- the optimiser of the PPO update on the flat weight block (no env-step code
// here): torch.optim.Adam with its defaults (no amsgrad, no weight decay) preceded by
// torch.nn.utils.clip_grad_norm_, on one slice [begin, begin + count) of the block, as one launch that
// also applies the update's stop rule (the reference's `if kl > target_kl: break`) on the device.
//
// One workgroup of 1024 threads strides over the slice (the PPO slices are at most 6 977 words; the
// entry point accepts up to 2^20).  Being the only workgroup it can decide and write the stop flag
// without a race: every thread reads the flag, the KL and the step word, a barrier follows, and only
// then thread 0 writes any of them.  The gradient kernels of cf2sim_ppo.hip only read the flag.
//
//   gate     ctrl[0] != 0: return, nothing written.  kl_summary[4] > target_kl (strict; a NaN
//            compares false): ctrl[0] = 1, return, nothing else written.
//   norm     sum g^2 in fp64: per thread in index order (stride 1024), then the wave by xor shuffles,
//            then the 16 wave sums in wave order from LDS.  Every thread ends with the same bits; the
//            geometry is fixed, so the same input gives the same bits.
//   update   per word, in fp64 from the fp32 values, each result rounded once to fp32:
//              g' = g min(1, max_grad_norm / (norm + 1e-6))                   (max_grad_norm > 0)
//              m  = b1 m + (1 - b1) g'          v = b2 v + (1 - b2) g'^2      (stored fp32)
//              w  = w - lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps)  (from the stored m, v)
//            b^t by repeated squaring in fp64 (exact for t = 1; a few ulp of fp64 otherwise).
//            The TU is compiled with -ffp-contract=off: the written formula is the arithmetic.
//            The gradient is read twice (norm, update); the second read hits the cache.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/cf2sim.h"
#include "cf2sim_internal.h"

namespace cf2 {

constexpr int ADAM_BLOCK = 1024, ADAM_WAVES = ADAM_BLOCK / 64;
constexpr uint32_t ADAM_MAX_COUNT = 1u << 20;

struct AdamArgs {
    float* w;                    // already offset by begin, like grad, m and v
    const float* grad;
    float* m;
    float* v;
    uint32_t* step;
    double* norm_out;
    const double* kl_summary;
    uint32_t* ctrl;
    uint32_t count;
    float lr, beta1, beta2, eps, max_grad_norm, target_kl;
};

__device__ __forceinline__ double powu(double b, uint32_t e) {
    double r = 1.0;
    for (; e; e >>= 1) {
        if (e & 1u) r *= b;
        b *= b;
    }
    return r;
}

// P members in one launch (cf2_adam_step_pop; adam_kernel<true>): workgroup k is member k's
// adam_kernel on the slice k `stride` floats further on, with its own step word, norm, KL summary and
// control block and with lr[k], max_grad_norm[k], target_kl[k].  It is the only writer of member k's
// words, so the argument of the header comment above holds per member.
struct AdamPopArgs {
    AdamArgs base;               // member 0's pointers; lr, max_grad_norm, target_kl unused
    size_t stride;               // floats between the members' blocks
    const float* lr;             // [P]
    const float* max_grad_norm;  // [P] or nullptr: no clipping
    const float* target_kl;      // [P] or nullptr: never read (no ctrl or no kl_summary)
};

// what a kernel instance is launched with and the AdamArgs its body sees; the stand-alone instance
// reads its own kernel argument, as before (cf2sim_ppo.hip, PpoKernelArgs, has the reason)
template <bool POP> struct AdamKernelArgs { using type = AdamArgs; };
template <> struct AdamKernelArgs<true> { using type = AdamPopArgs; };
__device__ __forceinline__ const AdamArgs& adam_args_of(const AdamArgs& a) { return a; }
__device__ __forceinline__ AdamArgs adam_args_of(const AdamPopArgs& p) {
    const uint32_t k = blockIdx.x;
    AdamArgs a = p.base;
    a.w += k * p.stride;
    a.grad += k * p.stride;
    a.m += k * p.stride;
    a.v += k * p.stride;
    a.step += k;
    if (a.norm_out) a.norm_out += k;
    if (a.kl_summary) a.kl_summary += 8u * (size_t)k;
    if (a.ctrl) a.ctrl += 4u * (size_t)k;
    a.lr = p.lr[k];
    a.max_grad_norm = p.max_grad_norm ? p.max_grad_norm[k] : 0.0f;
    a.target_kl = p.target_kl ? p.target_kl[k] : 0.0f;
    return a;
}

template <bool POP = false>
__global__ void __launch_bounds__(ADAM_BLOCK) adam_kernel(const typename AdamKernelArgs<POP>::type ka) {
    const AdamArgs a = adam_args_of(ka);
    __shared__ double wsum[ADAM_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool stopped = a.ctrl && a.ctrl[0] != 0u;
    const bool over = a.ctrl && a.kl_summary && a.kl_summary[4] > (double)a.target_kl;
    const uint32_t t = *a.step + 1u;
    __syncthreads();                 // every thread has read the flag, the KL and the step word
    if (stopped) return;
    if (over) {
        if (tid == 0) a.ctrl[0] = 1u;
        return;
    }

    double s = 0.0;
    for (uint32_t i = tid; i < a.count; i += ADAM_BLOCK) {
        const double g = (double)a.grad[i];
        s += g * g;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    double sq = 0.0;
#pragma unroll
    for (int w = 0; w < ADAM_WAVES; ++w) sq += wsum[w];
    const double norm = sqrt(sq);

    double coef = 1.0;
    if (a.max_grad_norm > 0.0f) {
        const double c = (double)a.max_grad_norm / (norm + 1e-6);
        coef = c > 1.0 ? 1.0 : c;    // a NaN norm gives a NaN factor, as torch's clamp does
    }
    const double b1 = (double)a.beta1, b2 = (double)a.beta2;
    const double step_size = (double)a.lr / (1.0 - powu(b1, t)), bc2_sqrt = sqrt(1.0 - powu(b2, t));
    const double omb1 = 1.0 - b1, omb2 = 1.0 - b2, eps = (double)a.eps;
    for (uint32_t i = tid; i < a.count; i += ADAM_BLOCK) {
        const double g = (double)a.grad[i] * coef;
        const float m = (float)(b1 * (double)a.m[i] + omb1 * g);
        const float v = (float)(b2 * (double)a.v[i] + omb2 * (g * g));
        const double denom = sqrt((double)v) / bc2_sqrt + eps;
        a.w[i] = (float)((double)a.w[i] - step_size * ((double)m / denom));
        a.m[i] = m;
        a.v[i] = v;
    }
    if (tid == 0) {
        *a.step = t;
        if (a.ctrl) a.ctrl[1] += 1u;
        if (a.norm_out) *a.norm_out = norm;
    }
}

static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

}  // namespace cf2

using namespace cf2;

extern "C" int cf2_adam_step(float* weights_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                             uint32_t begin, uint32_t count, uint32_t* step_dev, float lr, float beta1, float beta2,
                             float eps, float max_grad_norm, double* norm_out_dev, const double* kl_summary_dev,
                             float target_kl, uint32_t* ctrl_dev, void* stream) {
    if (count == 0) return CF2_OK;
    if (!weights_dev || !grad_dev || !exp_avg_dev || !exp_avg_sq_dev || !step_dev) return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(grad_dev, 4) || misaligned(exp_avg_dev, 4) ||
        misaligned(exp_avg_sq_dev, 4) || misaligned(step_dev, 4) || misaligned(ctrl_dev, 4) ||
        misaligned(norm_out_dev, 8) || misaligned(kl_summary_dev, 8))
        return CF2_ERR_INVALID_ARG;
    if ((uint64_t)begin + (uint64_t)count > 0xFFFFFFFFull || !(lr >= 0.0f) || !isfinite(lr)) return CF2_ERR_INVALID_ARG;
    if (count > ADAM_MAX_COUNT) return CF2_ERR_UNSUPPORTED;
    const AdamArgs a = {weights_dev + begin, grad_dev + begin, exp_avg_dev + begin, exp_avg_sq_dev + begin, step_dev,
                        norm_out_dev, kl_summary_dev, ctrl_dev, count, lr, beta1, beta2, eps, max_grad_norm, target_kl};
    hipLaunchKernelGGL(adam_kernel<false>, dim3(1), dim3(ADAM_BLOCK), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}

extern "C" int cf2_adam_step_pop(uint32_t members, float* weights_dev, const float* grad_dev, float* exp_avg_dev,
                                 float* exp_avg_sq_dev, size_t block_stride, uint32_t begin, uint32_t count,
                                 uint32_t* step_dev, const float* lr_dev, float beta1, float beta2, float eps,
                                 const float* max_grad_norm_dev, double* norm_out_dev, const double* kl_summary_dev,
                                 const float* target_kl_dev, uint32_t* ctrl_dev, void* stream) {
    if (count == 0 || members == 0) return CF2_OK;
    if (!weights_dev || !grad_dev || !exp_avg_dev || !exp_avg_sq_dev || !step_dev || !lr_dev ||
        (ctrl_dev && kl_summary_dev && !target_kl_dev))
        return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(grad_dev, 4) || misaligned(exp_avg_dev, 4) ||
        misaligned(exp_avg_sq_dev, 4) || misaligned(step_dev, 4) || misaligned(ctrl_dev, 4) || misaligned(lr_dev, 4) ||
        misaligned(max_grad_norm_dev, 4) || misaligned(target_kl_dev, 4) || misaligned(norm_out_dev, 8) ||
        misaligned(kl_summary_dev, 8))
        return CF2_ERR_INVALID_ARG;
    if ((uint64_t)begin + (uint64_t)count > 0xFFFFFFFFull || members >= (1u << 31)) return CF2_ERR_INVALID_ARG;
    if (count > ADAM_MAX_COUNT) return CF2_ERR_UNSUPPORTED;
    AdamPopArgs p = {};
    p.base = {weights_dev + begin, grad_dev + begin, exp_avg_dev + begin, exp_avg_sq_dev + begin, step_dev,
              norm_out_dev, kl_summary_dev, ctrl_dev, count, 0.0f, beta1, beta2, eps, 0.0f, 0.0f};
    p.stride = block_stride;
    p.lr = lr_dev, p.max_grad_norm = max_grad_norm_dev, p.target_kl = target_kl_dev;
    hipLaunchKernelGGL(adam_kernel<true>, dim3(members), dim3(ADAM_BLOCK), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}
