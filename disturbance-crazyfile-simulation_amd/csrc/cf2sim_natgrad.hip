// cf2sim_natgrad.hip -- the solver of the natural-gradient policy updates (NPG, TRPO) on the flat
// weight block (no env-step code here): conjugate gradients on (F + damping I) x = -grad with the
// Fisher-vector products of cf2_ppo_fisher_vec (cf2sim_ppo.hip), the step size from the KL target,
// and TRPO's backtracking line search, every scalar and every decision kept on the device.
//
// Every kernel follows adam_kernel (cf2sim_optim.hip): one workgroup of 1024 threads strides over the
// slice [begin, begin + count) of the flat blocks and writes nothing outside it.  Dot products are
// fp64 sums of fp64 products of the fp32 words, in a fixed order: per thread in index order (stride
// 1024), then the wave by xor shuffles, then the 16 wave sums in wave order from LDS, so every thread
// ends with the same bits and the same input gives the same bits.  Every word's update is evaluated
// in fp64 from the fp32 values and rounded once to fp32; a dot product that follows an update reads
// the rounded words.  The TU is compiled with -ffp-contract=off: the written formula is the
// arithmetic.  Being the only workgroup a kernel can read and write the scalars of ng_state and the
// stop flag without a race: every thread reads them, a barrier follows, and only then thread 0 writes.
//
// The cf2_ng_*_pop entry points launch the same bodies with one workgroup per member of a population
// (the <true> instances; NgCgPopArgs below).
//
// The rules (the reference's algs/npg and algs/trpo) are spelled out at the entry points in
// include/cf2sim.h; ng_state's layout is CF2_NG_* there.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/cf2sim.h"
#include "cf2sim_internal.h"

namespace cf2 {

constexpr int NG_BLOCK = 1024, NG_WAVES = NG_BLOCK / 64;
constexpr uint32_t NG_MAX_COUNT = 1u << 20;

// the block's sum of one double per thread; ends with a barrier-protected broadcast, so it can be
// called again at once
__device__ __forceinline__ double ng_block_sum(double s, double* wsum) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
    __syncthreads();                 // the previous call's readers are done with wsum
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < NG_WAVES; ++w) t += wsum[w];
    return t;
}

__device__ __forceinline__ double ng_powu(double b, uint32_t e) {
    double r = 1.0;
    for (; e; e >>= 1) {
        if (e & 1u) r *= b;
        b *= b;
    }
    return r;
}

struct NgCgArgs {
    const float* in;             // init: grad; step: z = F p          (all pointers offset by begin)
    float* b;                    // init only
    float* x;
    float* r;
    float* p;
    double* st;
    const uint32_t* gate;
    uint32_t count;
    float damping;
};

// P members in one launch (cf2_ng_*_pop; the <true> instances): workgroup k is member k's kernel on
// the blocks k `stride` floats further on, with ng_state + 16 k, the control block ctrl + 4 k and the
// member's own damping[k] and target_kl[k].  It is the only writer of member k's words (state, stop
// flag and weights among them) and never looks at another member's, so the header comment's argument
// holds per member.  `base` holds member 0's pointers; its damping and target_kl are unused.
struct NgCgPopArgs {
    NgCgArgs base;
    size_t stride;               // floats between the members' blocks
    const float* damping;        // [P]; nullptr (cg_init): not read
};

// what a kernel instance is launched with and the arguments its body sees; the stand-alone instance
// reads its own kernel argument, as before (cf2sim_ppo.hip, PpoKernelArgs, has the reason)
template <bool POP> struct NgCgKernelArgs { using type = NgCgArgs; };
template <> struct NgCgKernelArgs<true> { using type = NgCgPopArgs; };
__device__ __forceinline__ const NgCgArgs& ng_args_of(const NgCgArgs& a) { return a; }
__device__ __forceinline__ NgCgArgs ng_args_of(const NgCgPopArgs& p) {
    const uint32_t k = blockIdx.x;
    NgCgArgs a = p.base;
    a.in += k * p.stride;
    if (a.b) a.b += k * p.stride;
    a.x += k * p.stride;
    a.r += k * p.stride;
    a.p += k * p.stride;
    a.st += (size_t)CF2_NG_STATE_DOUBLES * k;
    if (a.gate) a.gate += 4u * (size_t)k;
    if (p.damping) a.damping = p.damping[k];
    return a;
}

template <bool POP = false>
__global__ void __launch_bounds__(NG_BLOCK) ng_cg_init_kernel(const typename NgCgKernelArgs<POP>::type ka) {
    const NgCgArgs a = ng_args_of(ka);
    __shared__ double wsum[NG_WAVES];
    const uint32_t tid = threadIdx.x;
    if (a.gate && a.gate[0] != 0u) return;
    double s = 0.0;
    for (uint32_t i = tid; i < a.count; i += NG_BLOCK) {
        const float b = -a.in[i];
        a.b[i] = b;
        a.x[i] = 0.0f;
        a.r[i] = b;
        a.p[i] = b;
        s += (double)b * (double)b;
    }
    const double bb = ng_block_sum(s, wsum);
    const int k = (int)tid;
    if (k < CF2_NG_STATE_DOUBLES) a.st[k] = (k == CF2_NG_RDOTR || k == CF2_NG_BDOTB || k == CF2_NG_RESIDUAL) ? bb : 0.0;
}

template <bool POP = false>
__global__ void __launch_bounds__(NG_BLOCK) ng_cg_step_kernel(const typename NgCgKernelArgs<POP>::type ka) {
    const NgCgArgs a = ng_args_of(ka);
    __shared__ double wsum[NG_WAVES];
    const uint32_t tid = threadIdx.x;
    const bool stopped = a.gate && a.gate[0] != 0u;
    const double rdotr = a.st[CF2_NG_RDOTR], steps = a.st[CF2_NG_CG_STEPS];
    const bool done = a.st[CF2_NG_CG_DONE] != 0.0;
    __syncthreads();                 // every thread has read the flag and the scalars
    if (stopped || done) return;
    const double damping = (double)a.damping;
    double s = 0.0;
    for (uint32_t i = tid; i < a.count; i += NG_BLOCK) {
        const double p = (double)a.p[i];
        s += p * ((double)a.in[i] + damping * p);
    }
    const double pz = ng_block_sum(s, wsum);
    const double alpha = rdotr / (pz + 1e-6);
    s = 0.0;
    for (uint32_t i = tid; i < a.count; i += NG_BLOCK) {
        const double p = (double)a.p[i];
        const double z = (double)a.in[i] + damping * p;
        a.x[i] = (float)((double)a.x[i] + alpha * p);
        const float r = (float)((double)a.r[i] - alpha * z);
        a.r[i] = r;
        s += (double)r * (double)r;
    }
    const double rr = ng_block_sum(s, wsum);
    const bool conv = sqrt(rr) < 1e-10;
    if (!conv) {
        const double beta = rr / (rdotr + 1e-6);
        for (uint32_t i = tid; i < a.count; i += NG_BLOCK) a.p[i] = (float)((double)a.r[i] + beta * (double)a.p[i]);
    }
    if (tid == 0) {
        a.st[CF2_NG_CG_STEPS] = steps + 1.0;
        a.st[CF2_NG_RESIDUAL] = rr;
        a.st[CF2_NG_PDOTZ] = pz;
        if (conv) a.st[CF2_NG_CG_DONE] = 1.0;
        else a.st[CF2_NG_RDOTR] = rr;
    }
}

struct NgDirArgs {
    const float* z;              // F x
    const float* x;
    const float* b;
    float* step;
    float* theta;
    float* theta_old;
    double* st;
    const uint32_t* gate;
    uint32_t count;
    float damping, target_kl;
};

struct NgDirPopArgs {
    NgDirArgs base;
    size_t stride;
    const float* damping;        // [P]
    const float* target_kl;      // [P]
};
template <bool POP> struct NgDirKernelArgs { using type = NgDirArgs; };
template <> struct NgDirKernelArgs<true> { using type = NgDirPopArgs; };
__device__ __forceinline__ const NgDirArgs& ng_args_of(const NgDirArgs& a) { return a; }
__device__ __forceinline__ NgDirArgs ng_args_of(const NgDirPopArgs& p) {
    const uint32_t k = blockIdx.x;
    NgDirArgs a = p.base;
    a.z += k * p.stride;
    a.x += k * p.stride;
    a.b += k * p.stride;
    a.step += k * p.stride;
    a.theta += k * p.stride;
    a.theta_old += k * p.stride;
    a.st += (size_t)CF2_NG_STATE_DOUBLES * k;
    if (a.gate) a.gate += 4u * (size_t)k;
    a.damping = p.damping[k];
    a.target_kl = p.target_kl[k];
    return a;
}

template <bool POP = false>
__global__ void __launch_bounds__(NG_BLOCK) ng_direction_kernel(const typename NgDirKernelArgs<POP>::type ka) {
    const NgDirArgs a = ng_args_of(ka);
    __shared__ double wsum[NG_WAVES];
    const uint32_t tid = threadIdx.x;
    if (a.gate && a.gate[0] != 0u) return;
    const double damping = (double)a.damping;
    double s = 0.0;
    for (uint32_t i = tid; i < a.count; i += NG_BLOCK) {
        const double x = (double)a.x[i];
        s += x * ((double)a.z[i] + damping * x);
    }
    const double xhx = ng_block_sum(s, wsum);
    const double alpha = sqrt(2.0 * (double)a.target_kl / (xhx + 1e-8));
    s = 0.0;
    for (uint32_t i = tid; i < a.count; i += NG_BLOCK) {
        const float st = (float)(alpha * (double)a.x[i]);
        const float th = a.theta[i];
        a.step[i] = st;
        a.theta_old[i] = th;
        a.theta[i] = (float)((double)th + (double)st);
        s += (double)a.b[i] * (double)st;
    }
    const double expected = ng_block_sum(s, wsum);
    if (tid == 0) {
        a.st[CF2_NG_XHX] = xhx;
        a.st[CF2_NG_ALPHA] = alpha;
        a.st[CF2_NG_EXPECTED] = expected;
    }
}

struct NgLsArgs {
    float* theta;
    const float* theta_old;
    const float* step;
    const double* eval;          // the policy summary of trial j
    const double* loss_before;
    double* st;
    uint32_t* ctrl;
    uint32_t count, j, total;
    float decay, target_kl;
};

struct NgLsPopArgs {
    NgLsArgs base;               // eval: [P][8]; loss_before: member 0's word
    size_t stride;
    size_t loss_before_stride;   // doubles between the members' loss_before words
    const float* target_kl;      // [P]
};
template <bool POP> struct NgLsKernelArgs { using type = NgLsArgs; };
template <> struct NgLsKernelArgs<true> { using type = NgLsPopArgs; };
__device__ __forceinline__ const NgLsArgs& ng_args_of(const NgLsArgs& a) { return a; }
__device__ __forceinline__ NgLsArgs ng_args_of(const NgLsPopArgs& p) {
    const uint32_t k = blockIdx.x;
    NgLsArgs a = p.base;
    a.theta += k * p.stride;
    a.theta_old += k * p.stride;
    a.step += k * p.stride;
    a.eval += 8u * (size_t)k;
    a.loss_before += k * p.loss_before_stride;
    a.st += (size_t)CF2_NG_STATE_DOUBLES * k;
    a.ctrl += 4u * (size_t)k;
    a.target_kl = p.target_kl[k];
    return a;
}

template <bool POP = false>
__global__ void __launch_bounds__(NG_BLOCK) ng_line_search_kernel(const typename NgLsKernelArgs<POP>::type ka) {
    const NgLsArgs a = ng_args_of(ka);
    const uint32_t tid = threadIdx.x;
    const bool stopped = a.ctrl[0] != 0u;
    const double loss = a.eval[1], kl = a.eval[4], before = *a.loss_before;
    __syncthreads();                 // every thread has read the flag and the three scalars
    if (stopped) return;
    const bool accept = isfinite(loss) && before - loss >= 0.0 && kl <= 1.5 * (double)a.target_kl;
    if (accept) {
        if (tid == 0) {
            a.ctrl[0] = 1u;
            a.ctrl[1] = a.j + 1u;
            a.st[CF2_NG_STEP_FRAC] = ng_powu((double)a.decay, a.j);
            a.st[CF2_NG_ACCEPT_STEP] = (double)(a.j + 1u);
            a.st[CF2_NG_LOSS_BEFORE] = before;
            a.st[CF2_NG_LOSS_AFTER] = loss;
            a.st[CF2_NG_KL_AFTER] = kl;
        }
        return;
    }
    if (a.j + 1u < a.total) {
        const double frac = ng_powu((double)a.decay, a.j + 1u);
        for (uint32_t i = tid; i < a.count; i += NG_BLOCK)
            a.theta[i] = (float)((double)a.theta_old[i] + frac * (double)a.step[i]);
        return;
    }
    for (uint32_t i = tid; i < a.count; i += NG_BLOCK) a.theta[i] = a.theta_old[i];
    if (tid == 0) {
        a.ctrl[0] = 1u;
        a.st[CF2_NG_STEP_FRAC] = 0.0;
        a.st[CF2_NG_ACCEPT_STEP] = 0.0;
        a.st[CF2_NG_LOSS_BEFORE] = before;
        a.st[CF2_NG_LOSS_AFTER] = before;
        a.st[CF2_NG_KL_AFTER] = 0.0;
    }
}

static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

// false: the slice is refused, *status is what the entry point returns
static bool ng_slice(uint32_t begin, uint32_t count, int* status) {
    if ((uint64_t)begin + (uint64_t)count > 0xFFFFFFFFull) *status = CF2_ERR_INVALID_ARG;
    else if (count > NG_MAX_COUNT) *status = CF2_ERR_UNSUPPORTED;
    else return true;
    return false;
}

static int ng_launched() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}

}  // namespace cf2

using namespace cf2;

extern "C" int cf2_ng_cg_init(const float* grad_dev, float* b_dev, float* x_dev, float* r_dev, float* p_dev, uint32_t begin,
                              uint32_t count, double* ng_state_dev, const uint32_t* ctrl_dev, void* stream) {
    if (count == 0) return CF2_OK;
    if (!grad_dev || !b_dev || !x_dev || !r_dev || !p_dev || !ng_state_dev) return CF2_ERR_INVALID_ARG;
    if (misaligned(grad_dev, 4) || misaligned(b_dev, 4) || misaligned(x_dev, 4) || misaligned(r_dev, 4) ||
        misaligned(p_dev, 4) || misaligned(ng_state_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    int status = CF2_OK;
    if (!ng_slice(begin, count, &status)) return status;
    const NgCgArgs a = {grad_dev + begin, b_dev + begin, x_dev + begin, r_dev + begin, p_dev + begin, ng_state_dev,
                        ctrl_dev, count, 0.0f};
    hipLaunchKernelGGL(ng_cg_init_kernel<false>, dim3(1), dim3(NG_BLOCK), 0, (hipStream_t)stream, a);
    return ng_launched();
}

extern "C" int cf2_ng_cg_step(const float* z_dev, float* x_dev, float* r_dev, float* p_dev, uint32_t begin, uint32_t count,
                              float damping, double* ng_state_dev, const uint32_t* ctrl_dev, void* stream) {
    if (count == 0) return CF2_OK;
    if (!z_dev || !x_dev || !r_dev || !p_dev || !ng_state_dev) return CF2_ERR_INVALID_ARG;
    if (misaligned(z_dev, 4) || misaligned(x_dev, 4) || misaligned(r_dev, 4) || misaligned(p_dev, 4) ||
        misaligned(ng_state_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (!(damping >= 0.0f) || !isfinite(damping)) return CF2_ERR_INVALID_ARG;
    int status = CF2_OK;
    if (!ng_slice(begin, count, &status)) return status;
    const NgCgArgs a = {z_dev + begin, nullptr, x_dev + begin, r_dev + begin, p_dev + begin, ng_state_dev, ctrl_dev,
                        count, damping};
    hipLaunchKernelGGL(ng_cg_step_kernel<false>, dim3(1), dim3(NG_BLOCK), 0, (hipStream_t)stream, a);
    return ng_launched();
}

extern "C" int cf2_ng_direction(const float* z_dev, const float* x_dev, const float* b_dev, float* step_dev,
                                float* weights_dev, float* weights_old_dev, uint32_t begin, uint32_t count,
                                float damping, float target_kl, double* ng_state_dev, const uint32_t* ctrl_dev,
                                void* stream) {
    if (count == 0) return CF2_OK;
    if (!z_dev || !x_dev || !b_dev || !step_dev || !weights_dev || !weights_old_dev || !ng_state_dev)
        return CF2_ERR_INVALID_ARG;
    if (misaligned(z_dev, 4) || misaligned(x_dev, 4) || misaligned(b_dev, 4) || misaligned(step_dev, 4) ||
        misaligned(weights_dev, 4) || misaligned(weights_old_dev, 4) || misaligned(ng_state_dev, 8) ||
        misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (!(damping >= 0.0f) || !isfinite(damping) || !(target_kl >= 0.0f) || !isfinite(target_kl))
        return CF2_ERR_INVALID_ARG;
    int status = CF2_OK;
    if (!ng_slice(begin, count, &status)) return status;
    const NgDirArgs a = {z_dev + begin, x_dev + begin, b_dev + begin, step_dev + begin, weights_dev + begin,
                         weights_old_dev + begin, ng_state_dev, ctrl_dev, count, damping, target_kl};
    hipLaunchKernelGGL(ng_direction_kernel<false>, dim3(1), dim3(NG_BLOCK), 0, (hipStream_t)stream, a);
    return ng_launched();
}

extern "C" int cf2_ng_line_search(float* weights_dev, const float* weights_old_dev, const float* step_dev, uint32_t begin,
                                  uint32_t count, uint32_t trial, uint32_t total, float decay, float target_kl,
                                  const double* eval_summary_dev, const double* loss_before_dev, double* ng_state_dev,
                                  uint32_t* ctrl_dev, void* stream) {
    if (count == 0) return CF2_OK;
    if (!weights_dev || !weights_old_dev || !step_dev || !eval_summary_dev || !loss_before_dev || !ng_state_dev ||
        !ctrl_dev)
        return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(weights_old_dev, 4) || misaligned(step_dev, 4) ||
        misaligned(eval_summary_dev, 8) || misaligned(loss_before_dev, 8) || misaligned(ng_state_dev, 8) ||
        misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (trial >= total || !(decay > 0.0f) || !(decay <= 1.0f) || !(target_kl >= 0.0f) || !isfinite(target_kl))
        return CF2_ERR_INVALID_ARG;
    int status = CF2_OK;
    if (!ng_slice(begin, count, &status)) return status;
    const NgLsArgs a = {weights_dev + begin, weights_old_dev + begin, step_dev + begin, eval_summary_dev, loss_before_dev,
                        ng_state_dev, ctrl_dev, count, trial, total, decay, target_kl};
    hipLaunchKernelGGL(ng_line_search_kernel<false>, dim3(1), dim3(NG_BLOCK), 0, (hipStream_t)stream, a);
    return ng_launched();
}

// ---- populations (include/cf2sim.h: "The four solver calls for a population")
// a population whose grid the launch cannot take
static bool ng_pop_overflows(uint32_t members) { return members >= (1u << 31); }

extern "C" int cf2_ng_cg_init_pop(uint32_t members, const float* grad_dev, float* b_dev, float* x_dev, float* r_dev,
                                  float* p_dev, size_t block_stride, uint32_t begin, uint32_t count,
                                  double* ng_state_dev, const uint32_t* ctrl_dev, void* stream) {
    if (count == 0 || members == 0) return CF2_OK;
    if (!grad_dev || !b_dev || !x_dev || !r_dev || !p_dev || !ng_state_dev) return CF2_ERR_INVALID_ARG;
    if (misaligned(grad_dev, 4) || misaligned(b_dev, 4) || misaligned(x_dev, 4) || misaligned(r_dev, 4) ||
        misaligned(p_dev, 4) || misaligned(ng_state_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (ng_pop_overflows(members)) return CF2_ERR_INVALID_ARG;
    int status = CF2_OK;
    if (!ng_slice(begin, count, &status)) return status;
    NgCgPopArgs p = {};
    p.base = {grad_dev + begin, b_dev + begin, x_dev + begin, r_dev + begin, p_dev + begin, ng_state_dev, ctrl_dev, count,
              0.0f};
    p.stride = block_stride;
    hipLaunchKernelGGL(ng_cg_init_kernel<true>, dim3(members), dim3(NG_BLOCK), 0, (hipStream_t)stream, p);
    return ng_launched();
}

extern "C" int cf2_ng_cg_step_pop(uint32_t members, const float* z_dev, float* x_dev, float* r_dev, float* p_dev,
                                  size_t block_stride, uint32_t begin, uint32_t count, const float* damping_dev,
                                  double* ng_state_dev, const uint32_t* ctrl_dev, void* stream) {
    if (count == 0 || members == 0) return CF2_OK;
    if (!z_dev || !x_dev || !r_dev || !p_dev || !damping_dev || !ng_state_dev) return CF2_ERR_INVALID_ARG;
    if (misaligned(z_dev, 4) || misaligned(x_dev, 4) || misaligned(r_dev, 4) || misaligned(p_dev, 4) ||
        misaligned(damping_dev, 4) || misaligned(ng_state_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (ng_pop_overflows(members)) return CF2_ERR_INVALID_ARG;
    int status = CF2_OK;
    if (!ng_slice(begin, count, &status)) return status;
    NgCgPopArgs p = {};
    p.base = {z_dev + begin, nullptr, x_dev + begin, r_dev + begin, p_dev + begin, ng_state_dev, ctrl_dev, count, 0.0f};
    p.stride = block_stride;
    p.damping = damping_dev;
    hipLaunchKernelGGL(ng_cg_step_kernel<true>, dim3(members), dim3(NG_BLOCK), 0, (hipStream_t)stream, p);
    return ng_launched();
}

extern "C" int cf2_ng_direction_pop(uint32_t members, const float* z_dev, const float* x_dev, const float* b_dev,
                                    float* step_dev, float* weights_dev, float* weights_old_dev, size_t block_stride,
                                    uint32_t begin, uint32_t count, const float* damping_dev, const float* target_kl_dev,
                                    double* ng_state_dev, const uint32_t* ctrl_dev, void* stream) {
    if (count == 0 || members == 0) return CF2_OK;
    if (!z_dev || !x_dev || !b_dev || !step_dev || !weights_dev || !weights_old_dev || !damping_dev || !target_kl_dev ||
        !ng_state_dev)
        return CF2_ERR_INVALID_ARG;
    if (misaligned(z_dev, 4) || misaligned(x_dev, 4) || misaligned(b_dev, 4) || misaligned(step_dev, 4) ||
        misaligned(weights_dev, 4) || misaligned(weights_old_dev, 4) || misaligned(damping_dev, 4) ||
        misaligned(target_kl_dev, 4) || misaligned(ng_state_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (ng_pop_overflows(members)) return CF2_ERR_INVALID_ARG;
    int status = CF2_OK;
    if (!ng_slice(begin, count, &status)) return status;
    NgDirPopArgs p = {};
    p.base = {z_dev + begin, x_dev + begin, b_dev + begin, step_dev + begin, weights_dev + begin, weights_old_dev + begin,
              ng_state_dev, ctrl_dev, count, 0.0f, 0.0f};
    p.stride = block_stride;
    p.damping = damping_dev, p.target_kl = target_kl_dev;
    hipLaunchKernelGGL(ng_direction_kernel<true>, dim3(members), dim3(NG_BLOCK), 0, (hipStream_t)stream, p);
    return ng_launched();
}

extern "C" int cf2_ng_line_search_pop(uint32_t members, float* weights_dev, const float* weights_old_dev,
                                      const float* step_dev, size_t block_stride, uint32_t begin, uint32_t count,
                                      uint32_t trial, uint32_t total, float decay, const float* target_kl_dev,
                                      const double* eval_summary_dev, const double* loss_before_dev,
                                      size_t loss_before_stride, double* ng_state_dev, uint32_t* ctrl_dev, void* stream) {
    if (count == 0 || members == 0) return CF2_OK;
    if (!weights_dev || !weights_old_dev || !step_dev || !target_kl_dev || !eval_summary_dev || !loss_before_dev ||
        !ng_state_dev || !ctrl_dev)
        return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(weights_old_dev, 4) || misaligned(step_dev, 4) ||
        misaligned(target_kl_dev, 4) || misaligned(eval_summary_dev, 8) || misaligned(loss_before_dev, 8) ||
        misaligned(ng_state_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (trial >= total || !(decay > 0.0f) || !(decay <= 1.0f)) return CF2_ERR_INVALID_ARG;
    if (ng_pop_overflows(members)) return CF2_ERR_INVALID_ARG;
    int status = CF2_OK;
    if (!ng_slice(begin, count, &status)) return status;
    NgLsPopArgs p = {};
    p.base = {weights_dev + begin, weights_old_dev + begin, step_dev + begin, eval_summary_dev, loss_before_dev,
              ng_state_dev, ctrl_dev, count, trial, total, decay, 0.0f};
    p.stride = block_stride;
    p.loss_before_stride = loss_before_stride;
    p.target_kl = target_kl_dev;
    hipLaunchKernelGGL(ng_line_search_kernel<true>, dim3(members), dim3(NG_BLOCK), 0, (hipStream_t)stream, p);
    return ng_launched();
}
