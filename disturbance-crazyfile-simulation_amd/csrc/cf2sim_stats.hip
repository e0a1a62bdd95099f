// cf2sim_stats.hip -- per-epoch training statistics over the rollout buffers collect() leaves on
// the device (no env-step code here).
//
// (a) Episode statistics.  The reference's roll_out (algs/iwpg/iwpg.py:372-410) keeps ep_ret, ep_costs
//     and ep_len per env and, at every episode end, does logger.store(EpRet=, EpLen=, EpCosts=); the
//     epoch log then prints their mean / std / min / max.  Here the envs auto-reset inside the step
//     kernel and an episode (500 steps) spans many collects (T = 32...64), so the running sums are a
//     per-env carry the caller keeps between calls.  One thread per env scans [T, n] forward in
//     time; a finished episode's three values go to the optional per-slot outputs and into the
//     thread's accumulators (count; sum, sum of squares, min, max of each), which are reduced wave
//     shuffle -> LDS -> one partial per block -> a finalize launch, all in a fixed order: the same
//     input gives the same bits.  The carries add plain f32 / int32 in time order, so splitting a
//     rollout into several calls changes no carry and no episode value.
//
// (b) Column moments of a dense [rows, D] f32 matrix: per column the mean and M2 = sum (x - mean)^2,
//     the batch moments of OnlineMeanStd.update (utils/online_mean_std.py), read once.  The matrix
//     is streamed as a flat array of V-float vectors (V = 4, 2 or 1 by the base's alignment).  A
//     block works through a contiguous chunk that starts on a row boundary, A vectors per
//     iteration, A the largest multiple of the column period D / gcd(V, D) that fits 256 threads:
//     the columns of a lane's vector never change, so its shifted fp64 sums sum (x - p),
//     sum (x - p)^2 stay in registers (p = the chunk's first row; x - p is exact in fp64 for f32
//     values within a factor 2^29 of each other, so a column with a large mean and a small spread
//     loses nothing).  Block partials (count, mean, M2)
//     go to scratch; a finalize launch merges them pairwise in index order (Chan et al.).  No
//     atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cf2sim.h"
#include "cf2sim_internal.h"

namespace cf2 {

// ---------------------------------------------------------------------------------------------
// (a) episode statistics
// ---------------------------------------------------------------------------------------------
constexpr int EP_BLOCK = 256;
constexpr int EP_WORDS = 16;                  // doubles per partial and in the summary

struct Moments {                              // of one of return / length / cost
    double sum, sumsq, mn, mx;
    __device__ void clear() { sum = 0.0; sumsq = 0.0; mn = __builtin_inf(); mx = -__builtin_inf(); }
    __device__ void add(double v) { sum += v; sumsq += v * v; mn = fmin(mn, v); mx = fmax(mx, v); }
    __device__ void merge(const Moments& o) { sum += o.sum; sumsq += o.sumsq; mn = fmin(mn, o.mn); mx = fmax(mx, o.mx); }
    __device__ Moments shifted_down(int d) const {
        Moments o;
        o.sum = __shfl_down(sum, d); o.sumsq = __shfl_down(sumsq, d); o.mn = __shfl_down(mn, d); o.mx = __shfl_down(mx, d);
        return o;
    }
    __device__ void load(const double* p) { sum = p[0]; sumsq = p[1]; mn = p[2]; mx = p[3]; }
    __device__ void store(double* p) const { p[0] = sum; p[1] = sumsq; p[2] = mn; p[3] = mx; }
};

struct EpAcc {
    double count;
    Moments ret, len, cost;
    __device__ void clear() { count = 0.0; ret.clear(); len.clear(); cost.clear(); }
    __device__ void merge(const EpAcc& o) { count += o.count; ret.merge(o.ret); len.merge(o.len); cost.merge(o.cost); }
    // summary layout (include/cf2sim.h cf2_episode_stats)
    __device__ void load(const double* p) { count = p[0]; ret.load(p + 1); len.load(p + 5); cost.load(p + 9); }
    __device__ void store(double* p) const {
        p[0] = count; ret.store(p + 1); len.store(p + 5); cost.store(p + 9);
        p[13] = 0.0; p[14] = 0.0; p[15] = 0.0;
    }
};

// every thread of the block calls this; thread 0 returns the block's total (lane order inside a
// wave, then wave order: fixed)
__device__ void ep_block_reduce(EpAcc& a, double* lds /* [EP_BLOCK / 64][EP_WORDS] */) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        EpAcc o;
        o.count = __shfl_down(a.count, d);
        o.ret = a.ret.shifted_down(d);
        o.len = a.len.shifted_down(d);
        o.cost = a.cost.shifted_down(d);
        a.merge(o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) a.store(lds + wave * EP_WORDS);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < EP_BLOCK / 64; ++w) {
            EpAcc o;
            o.load(lds + w * EP_WORDS);
            a.merge(o);
        }
    }
}

__global__ void __launch_bounds__(EP_BLOCK) episode_stats_kernel(
        uint32_t T, uint32_t n, const float* __restrict__ rew, const float* __restrict__ cost,
        const uint8_t* __restrict__ done, float* __restrict__ carry_ret, float* __restrict__ carry_cost,
        int32_t* __restrict__ carry_len, float* __restrict__ ep_ret_out, int32_t* __restrict__ ep_len_out,
        float* __restrict__ ep_cost_out, double* __restrict__ partial) {
    __shared__ double lds[(EP_BLOCK / 64) * EP_WORDS];
    const uint32_t e = blockIdx.x * EP_BLOCK + threadIdx.x;
    const bool live = e < n;
    const uint32_t ec = live ? e : n - 1;             // idle lanes read a valid column and write nothing
    EpAcc acc;
    acc.clear();
    float er = carry_ret[ec], ecst = carry_cost[ec];
    int32_t el = carry_len[ec];
    // the scan is serial in t; the loads of U steps are issued together (as gae_kernel does)
    constexpr uint32_t U = 8;
    for (uint32_t t0 = 0; t0 < T; t0 += U) {
        float rr[U], cc[U];
        uint8_t dd[U];
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            const uint32_t t = t0 + j < T ? t0 + j : T - 1;
            const size_t k = (size_t)t * n + ec;
            rr[j] = rew[k];
            cc[j] = cost ? cost[k] : 0.0f;
            dd[j] = done[k];
        }
        __builtin_amdgcn_sched_barrier(0);      // the loads stay ahead of the scan
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            if (t0 + j >= T) break;
            er += rr[j];
            ecst += cc[j];
            ++el;
            if (dd[j] != 0) {
                if (live) {
                    const size_t k = (size_t)(t0 + j) * n + e;
                    if (ep_ret_out) ep_ret_out[k] = er;
                    if (ep_len_out) ep_len_out[k] = el;
                    if (ep_cost_out) ep_cost_out[k] = ecst;
                    acc.count += 1.0;
                    acc.ret.add((double)er);
                    acc.len.add((double)el);
                    acc.cost.add((double)ecst);
                }
                er = 0.0f;
                ecst = 0.0f;
                el = 0;
            }
        }
    }
    if (live) {
        carry_ret[e] = er;
        carry_cost[e] = ecst;
        carry_len[e] = el;
    }
    ep_block_reduce(acc, lds);
    if (threadIdx.x == 0) acc.store(partial + (size_t)blockIdx.x * EP_WORDS);
}

// one block: thread i merges partials i, i + 256, ... in that order (four loaded at a time), then
// the block reduction
__global__ void __launch_bounds__(EP_BLOCK) episode_stats_finalize_kernel(const double* __restrict__ partial,
                                                                          uint32_t nblocks, int accumulate,
                                                                          double* __restrict__ summary) {
    __shared__ double lds[(EP_BLOCK / 64) * EP_WORDS];
    EpAcc acc;
    acc.clear();
    constexpr uint32_t R = 4;                    // partials loaded together
    for (uint32_t b0 = threadIdx.x; b0 < nblocks; b0 += R * EP_BLOCK) {
        EpAcc o[R];
#pragma unroll
        for (uint32_t k = 0; k < R; ++k) {
            const uint32_t b = b0 + k * EP_BLOCK;
            o[k].load(partial + (size_t)(b < nblocks ? b : b0) * EP_WORDS);
            if (b >= nblocks) o[k].clear();
        }
#pragma unroll
        for (uint32_t k = 0; k < R; ++k) acc.merge(o[k]);
    }
    ep_block_reduce(acc, lds);
    if (threadIdx.x == 0) {
        if (accumulate && summary[0] > 0.0) {       // a summary with count 0 is empty whatever it holds
            EpAcc old;
            old.load(summary);
            old.merge(acc);
            acc = old;
        }
        if (!(acc.count > 0.0)) acc.clear();
        acc.store(summary);
    }
}

// ---------------------------------------------------------------------------------------------
// (b) column moments
// ---------------------------------------------------------------------------------------------
constexpr int CM_BLOCK = 256;
constexpr uint32_t CM_MAX_BLOCKS = 2048;      // scratch is sized for this many block partials
constexpr uint32_t CM_MAX_D = 64;
constexpr int CM_UNROLL = 8;                  // vector loads in flight per lane

template <int V> struct VecOf;
template <> struct VecOf<1> { typedef float type; };
template <> struct VecOf<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct VecOf<4> { typedef float type __attribute__((ext_vector_type(4))); };

template <int V> __device__ inline float vec_get(const typename VecOf<V>::type& v, int j) { return v[j]; }
template <> __device__ inline float vec_get<1>(const float& v, int) { return v; }

__host__ __device__ constexpr uint32_t cm_gcd(uint32_t a, uint32_t b) { return b == 0 ? a : cm_gcd(b, a % b); }
// vectors a block consumes per iteration: the lanes' columns repeat with period D / gcd(V, D)
__host__ __device__ constexpr uint32_t cm_active(uint32_t V, uint32_t D) {
    return CM_BLOCK - CM_BLOCK % (D / cm_gcd(V, D));
}

struct CmGeom {
    uint64_t nvec;        // whole vectors in the matrix
    uint64_t iters;       // block iterations of A vectors that cover them
    uint64_t per_block;   // iterations per block
    uint32_t blocks;
};

static CmGeom cm_geometry(uint64_t rows, uint32_t D, uint32_t V, uint32_t max_blocks) {
    CmGeom g;
    const uint64_t A = cm_active(V, D);
    g.nvec = rows * D / V;
    g.iters = (g.nvec + A - 1) / A;
    if (g.iters == 0) g.iters = 1;            // fewer than V elements: the tail code handles them
    g.per_block = (g.iters + max_blocks - 1) / max_blocks;
    if (g.per_block < (uint64_t)CM_UNROLL) g.per_block = CM_UNROLL;   // a block's loads go out CM_UNROLL at a time
    g.blocks = (uint32_t)((g.iters + g.per_block - 1) / g.per_block);
    return g;
}

// partial layout: scratch[(c * CM_MAX_BLOCKS + b) * 3 + {0, 1, 2}] = count, mean, M2 of column c in
// block b (a column's partials are contiguous for the finalize launch)
template <int V>
__global__ void __launch_bounds__(CM_BLOCK) column_moments_kernel(const float* __restrict__ x, uint64_t rows,
                                                                  uint32_t D, uint64_t nvec, uint64_t per_block,
                                                                  double* __restrict__ partial) {
    typedef typename VecOf<V>::type vec_t;
    __shared__ double s1s[CM_BLOCK * V], s2s[CM_BLOCK * V];
    const uint32_t A = cm_active(V, D);
    const uint32_t tid = threadIdx.x;
    const uint64_t total = rows * D;
    const uint64_t v_begin = (uint64_t)blockIdx.x * per_block * A;       // a row boundary: A V % D == 0
    uint64_t v_end = v_begin + per_block * A;
    if (v_end > nvec) v_end = nvec;
    const bool last = blockIdx.x == gridDim.x - 1;
    const uint64_t e_begin = v_begin * V;                                 // first element of the chunk
    const uint64_t e_end = last ? total : v_end * V;                      // the last block takes the tail
    const vec_t* xv = reinterpret_cast<const vec_t*>(x);

    double p[V], s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const uint32_t c = (tid * V + j) % D;                             // this slot's column, fixed
        p[j] = e_begin + c < total ? (double)x[e_begin + c] : 0.0;        // the chunk's first row
        s1[j] = 0.0;
        s2[j] = 0.0;
    }
    if (tid < A) {
        uint64_t v = v_begin + tid;
        for (; v + (uint64_t)(CM_UNROLL - 1) * A < v_end; v += (uint64_t)CM_UNROLL * A) {
            vec_t q[CM_UNROLL];
#pragma unroll
            for (int k = 0; k < CM_UNROLL; ++k) q[k] = __builtin_nontemporal_load(xv + v + (uint64_t)k * A);
            // keep the loads together: left alone, the scheduler spreads them through the sums below
            // to save registers and two or three are in flight per wave instead of CM_UNROLL
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < CM_UNROLL; ++k) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const double d = (double)vec_get<V>(q[k], j) - p[j];
                    s1[j] += d;
                    s2[j] = fma(d, d, s2[j]);
                }
            }
        }
        for (; v < v_end; v += A) {
            const vec_t q = __builtin_nontemporal_load(xv + v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double d = (double)vec_get<V>(q, j) - p[j];
                s1[j] += d;
                s2[j] = fma(d, d, s2[j]);
            }
        }
    }
    // block reduction per column, fixed order.  Slot q = tid V + j holds column q % D; thread
    // r = g D + c sums the slots c + D (g + G k) (k = 0, 1, ...), then thread c the G group sums.
#pragma unroll
    for (int j = 0; j < V; ++j) {
        s1s[tid * V + j] = s1[j];
        s2s[tid * V + j] = s2[j];
    }
    __syncthreads();
    const uint32_t G = CM_BLOCK / D, slots = A * V;
    double a1 = 0.0, a2 = 0.0;
    if (tid < G * D) {
        const uint32_t c = tid % D, g = tid / D;
        for (uint32_t q = c + D * g; q < slots; q += D * G) {
            a1 += s1s[q];
            a2 += s2s[q];
        }
    }
    __syncthreads();                    // every slot is read: the group sums go where the slots were
    s1s[tid] = a1;
    s2s[tid] = a2;
    __syncthreads();
    if (tid < D) {
        a1 = 0.0;
        a2 = 0.0;
        for (uint32_t g = 0; g < G; ++g) {
            a1 += s1s[g * D + tid];
            a2 += s2s[g * D + tid];
        }
        // rows of the chunk that hold column tid (every whole row, and the tail's columns)
        const uint64_t r0 = e_begin / D, full = e_end / D, rem = e_end % D;
        const double cnt = (double)(full - r0 + (tid < rem ? 1u : 0u));
        const double pc = e_begin + tid < total ? (double)x[e_begin + tid] : 0.0;
        if (last) {                     // the elements past the last whole vector (fewer than V)
            for (uint64_t e = nvec * V; e < total; ++e) {
                if (e % D != tid) continue;
                const double d = (double)x[e] - pc;
                a1 += d;
                a2 = fma(d, d, a2);
            }
        }
        double mean = 0.0, m2 = 0.0;
        if (cnt > 0.0) {
            // p is a sample of the column, so a1^2 / cnt is of a2's size at most and the difference
            // keeps its digits; the clamp only guards the last bit (M2 >= 0)
            mean = pc + a1 / cnt;
            m2 = fmax(a2 - a1 * a1 / cnt, 0.0);
        }
        double* o = partial + ((size_t)tid * CM_MAX_BLOCKS + blockIdx.x) * 3;
        o[0] = cnt;
        o[1] = mean;
        o[2] = m2;
    }
}

struct CmPart { double n, mean, m2; };

// Chan et al.: b (the later rows) merged into a
__device__ inline void cm_merge(CmPart& a, const CmPart& b) {
    if (b.n == 0.0) return;
    if (a.n == 0.0) { a = b; return; }
    const double nab = a.n + b.n, delta = b.mean - a.mean;
    a.mean = a.mean + delta * (b.n / nab);
    a.m2 = a.m2 + b.m2 + delta * delta * (a.n * b.n / nab);
    a.n = nab;
}

// one block per column: thread i merges the (at most CM_RUN) partials of blocks i per, ..., in
// index order, their loads issued together; the 256 runs are then merged pairwise, neighbours first,
// by a tree whose shape depends on the block count only.  (One thread per column walking all the
// partials waits for memory once per partial: ~100 us at 2048 partials.)
constexpr uint32_t CM_RUN = CM_MAX_BLOCKS / CM_BLOCK;
__global__ void __launch_bounds__(CM_BLOCK) column_moments_finalize_kernel(const double* __restrict__ partial,
                                                                           uint32_t nblocks, uint32_t D,
                                                                           double* __restrict__ out) {
    __shared__ CmPart parts[CM_BLOCK];
    const uint32_t tid = threadIdx.x, c = blockIdx.x;
    const uint32_t per = (nblocks + CM_BLOCK - 1) / CM_BLOCK;            // <= CM_RUN
    const double* col = partial + (size_t)c * CM_MAX_BLOCKS * 3;
    CmPart run[CM_RUN];
#pragma unroll
    for (uint32_t k = 0; k < CM_RUN; ++k) {
        const uint32_t b = tid * per + k;
        const bool have = k < per && b < nblocks;
        const double* q = col + (size_t)(have ? b : 0) * 3;
        run[k].n = have ? q[0] : 0.0;
        run[k].mean = q[1];
        run[k].m2 = q[2];
    }
    CmPart a = {0.0, 0.0, 0.0};
#pragma unroll
    for (uint32_t k = 0; k < CM_RUN; ++k) cm_merge(a, run[k]);            // skips the empty ones
    parts[tid] = a;
    __syncthreads();
    for (uint32_t s = 1; s < CM_BLOCK; s <<= 1) {
        if (tid % (2 * s) == 0) {
            a = parts[tid];
            cm_merge(a, parts[tid + s]);
            parts[tid] = a;
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[c] = parts[0].mean;
        out[D + c] = parts[0].m2;
    }
}

// vector width the matrix is streamed with: what the base's alignment allows (a vector may
// straddle rows; its slots' columns are fixed all the same)
static uint32_t cm_vector_width(const float* x) {
    return ((uintptr_t)x & 15u) == 0 ? 4u : ((uintptr_t)x & 7u) == 0 ? 2u : 1u;
}

static uint32_t cm_max_blocks() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint32_t want = (uint32_t)(cus > 0 ? cus : 256) * 8u;           // 8 blocks of 4 waves per CU
    return want < CM_MAX_BLOCKS ? want : CM_MAX_BLOCKS;
}

}  // namespace cf2

using namespace cf2;

extern "C" size_t cf2_episode_stats_scratch_bytes(uint32_t n) {
    return (size_t)((n + EP_BLOCK - 1) / EP_BLOCK) * EP_WORDS * sizeof(double);
}

extern "C" int cf2_episode_stats(uint32_t T, uint32_t n, const float* rew_dev, const float* cost_dev,
                                 const uint8_t* done_dev, float* carry_ret_dev, float* carry_cost_dev,
                                 int32_t* carry_len_dev, float* ep_ret_out_dev, int32_t* ep_len_out_dev,
                                 float* ep_cost_out_dev, double* summary_dev, int accumulate, void* scratch_dev,
                                 void* stream) {
    if (T == 0 || n == 0) return CF2_OK;
    if (!rew_dev || !done_dev || !carry_ret_dev || !carry_cost_dev || !carry_len_dev || !summary_dev || !scratch_dev)
        return CF2_ERR_INVALID_ARG;
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t blocks = (n + EP_BLOCK - 1) / EP_BLOCK;
    double* partial = static_cast<double*>(scratch_dev);
    hipLaunchKernelGGL(episode_stats_kernel, dim3(blocks), dim3(EP_BLOCK), 0, s, T, n, rew_dev, cost_dev, done_dev,
                       carry_ret_dev, carry_cost_dev, carry_len_dev, ep_ret_out_dev, ep_len_out_dev, ep_cost_out_dev,
                       partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(episode_stats_finalize_kernel, dim3(1), dim3(EP_BLOCK), 0, s, partial, blocks, accumulate,
                       summary_dev);
    e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}

extern "C" size_t cf2_column_moments_scratch_bytes(uint64_t rows, uint32_t D) {
    if (rows == 0 || D == 0 || D > CM_MAX_D) return 0;
    return (size_t)CM_MAX_BLOCKS * D * 3 * sizeof(double);
}

extern "C" int cf2_column_moments(const float* x_dev, uint64_t rows, uint32_t D, double* out_dev, void* scratch_dev,
                                  void* stream) {
    if (D == 0 || D > CM_MAX_D) return CF2_ERR_INVALID_ARG;
    if (rows == 0) return CF2_OK;
    if (!x_dev || !out_dev || !scratch_dev || ((uintptr_t)x_dev & 3u) || rows > (UINT64_MAX >> 8) / D)
        return CF2_ERR_INVALID_ARG;
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t V = cm_vector_width(x_dev);
    const CmGeom g = cm_geometry(rows, D, V, cm_max_blocks());
    double* partial = static_cast<double*>(scratch_dev);
    const dim3 grid(g.blocks), block(CM_BLOCK);
    if (V == 4)
        hipLaunchKernelGGL(column_moments_kernel<4>, grid, block, 0, s, x_dev, rows, D, g.nvec, g.per_block, partial);
    else if (V == 2)
        hipLaunchKernelGGL(column_moments_kernel<2>, grid, block, 0, s, x_dev, rows, D, g.nvec, g.per_block, partial);
    else
        hipLaunchKernelGGL(column_moments_kernel<1>, grid, block, 0, s, x_dev, rows, D, g.nvec, g.per_block, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(column_moments_finalize_kernel, dim3(D), dim3(CM_BLOCK), 0, s, partial, g.blocks, D, out_dev);
    e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}
