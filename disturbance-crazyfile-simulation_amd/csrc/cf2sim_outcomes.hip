// cf2sim_outcomes.hip -- per-level episode outcomes over the rollout buffers (no env-step code here).
//
// The reference logs, with every finished episode, the disturbance level it ran under
// (episodic_data.csv: episode, disturbance level, steps, return) and evaluates a policy per level
// (utils/evaluation.py).  cf2_episode_stats (cf2sim_stats.hip) pools every episode into one
// summary; here the same scan bins the finished episodes by their level and tells a crash from a
// time-out.  Three launches on the caller's stream:
//   1. scan: one thread per env walks [T, n] forward in time with the per-env carries of
//      cf2_episode_stats (plain f32 / int32 adds in time order, so splitting a rollout over several
//      calls changes no carry and no episode value).  Per slot it writes one tag byte into scratch:
//      0xFF where no episode was recorded, else the bin (bits 0-5) and the crash / time-out flags
//      (bits 6, 7); a recorded episode's return, cost and length go to the slot's record words.
//   2. reduce, one block per chunk of slots: the block reads its tags once (four per load) and, 1024
//      slots at a time, compacts the recorded episodes in slot order into an LDS list (wave scan,
//      then wave order); lane b < L + 1 walks the list and adds the episodes of bin b to its fp64
//      accumulators, so a bin's sum is taken in slot order and needs no cross-lane reduction.  One
//      partial per (bin, chunk).  (A grid of (chunk, bin) blocks that each reduced one bin by
//      shuffles re-read the tags L + 1 times and took 228 us at [32, 262 144] against 28 us of
//      cf2_episode_stats: the blocks spent their time in the 15-value fp64 shuffle reduction.)
//   3. finalize, one block per bin: the bin's partials in chunk order, then the table row.
// No atomics; the geometry depends on (T, n) only: the same input gives the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cf2sim.h"
#include "cf2sim_internal.h"

namespace cf2 {

constexpr int OC_BLOCK = 256;
constexpr int OC_WORDS = 16;                  // doubles per partial and per table row
constexpr uint32_t OC_TAGS = 4;               // tag bytes per load of the reduce kernel
constexpr uint32_t OC_UNROLL = 4;             // tag loads in flight per lane
constexpr uint64_t OC_SPAN = (uint64_t)OC_BLOCK * OC_TAGS;             // slots a block covers per load round
constexpr uint32_t OC_MAX_CHUNKS = 1024;
constexpr uint32_t OC_NONE = 0xFFu, OC_CRASH = 0x40u, OC_TIMEOUT = 0x80u, OC_BIN = 0x3Fu;

struct OcMoments {                            // of one of return / length / cost
    double sum, sumsq, mn, mx;
    __device__ void clear() { sum = 0.0; sumsq = 0.0; mn = __builtin_inf(); mx = -__builtin_inf(); }
    __device__ void add(double v) { sum += v; sumsq += v * v; mn = fmin(mn, v); mx = fmax(mx, v); }
    __device__ void merge(const OcMoments& o) { sum += o.sum; sumsq += o.sumsq; mn = fmin(mn, o.mn); mx = fmax(mx, o.mx); }
    __device__ OcMoments shifted_down(int d) const {
        OcMoments o;
        o.sum = __shfl_down(sum, d); o.sumsq = __shfl_down(sumsq, d); o.mn = __shfl_down(mn, d); o.mx = __shfl_down(mx, d);
        return o;
    }
    __device__ void load(const double* p) { sum = p[0]; sumsq = p[1]; mn = p[2]; mx = p[3]; }
    __device__ void store(double* p) const { p[0] = sum; p[1] = sumsq; p[2] = mn; p[3] = mx; }
};

struct OcAcc {
    double count, crashes, timeouts;
    OcMoments ret, len, cost;
    __device__ void clear() { count = 0.0; crashes = 0.0; timeouts = 0.0; ret.clear(); len.clear(); cost.clear(); }
    __device__ void merge(const OcAcc& o) {
        count += o.count; crashes += o.crashes; timeouts += o.timeouts;
        ret.merge(o.ret); len.merge(o.len); cost.merge(o.cost);
    }
    // row layout (include/cf2sim.h cf2_level_outcomes)
    __device__ void load(const double* p) {
        count = p[0]; ret.load(p + 1); len.load(p + 5); cost.load(p + 9); crashes = p[13]; timeouts = p[14];
    }
    __device__ void store(double* p) const {
        p[0] = count; ret.store(p + 1); len.store(p + 5); cost.store(p + 9);
        p[13] = crashes; p[14] = timeouts; p[15] = 0.0;
    }
};

// every thread of the block calls this; thread 0 returns the block's total (lane order inside a
// wave, then wave order: fixed)
__device__ void oc_block_reduce(OcAcc& a, double* lds /* [OC_BLOCK / 64][OC_WORDS] */) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        OcAcc o;
        o.count = __shfl_down(a.count, d);
        o.crashes = __shfl_down(a.crashes, d);
        o.timeouts = __shfl_down(a.timeouts, d);
        o.ret = a.ret.shifted_down(d);
        o.len = a.len.shifted_down(d);
        o.cost = a.cost.shifted_down(d);
        a.merge(o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) a.store(lds + wave * OC_WORDS);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < OC_BLOCK / 64; ++w) {
            OcAcc o;
            o.load(lds + w * OC_WORDS);
            a.merge(o);
        }
    }
}

// Scratch: the per-slot records (return f32, cost f32, length int32, [T n] each), the tag bytes
// (rounded up to 8) and the reduce kernel's partials [L + 1][chunks][OC_WORDS].
struct OcGeom {
    uint64_t slots;        // T n
    uint64_t per_chunk;    // slots per reduce block, a multiple of OC_SPAN
    uint32_t chunks;
    size_t off_cost, off_len, off_tag, off_partial, bytes;
};

static OcGeom oc_geometry(uint32_t T, uint32_t n, uint32_t L) {
    OcGeom g;
    g.slots = (uint64_t)T * n;
    const uint64_t unit = OC_SPAN * OC_UNROLL;                         // a block's loads go out OC_UNROLL at a time
    uint64_t chunks = (g.slots + unit - 1) / unit;
    if (chunks > OC_MAX_CHUNKS) chunks = OC_MAX_CHUNKS;
    if (chunks == 0) chunks = 1;
    g.per_chunk = ((g.slots + chunks - 1) / chunks + OC_SPAN - 1) / OC_SPAN * OC_SPAN;
    if (g.per_chunk == 0) g.per_chunk = OC_SPAN;
    g.chunks = (uint32_t)((g.slots + g.per_chunk - 1) / g.per_chunk);
    if (g.chunks == 0) g.chunks = 1;
    g.off_cost = (size_t)g.slots * 4;
    g.off_len = (size_t)g.slots * 8;
    g.off_tag = (size_t)g.slots * 12;                                  // 4-byte aligned: the tags are read as words
    g.off_partial = (g.off_tag + (size_t)g.slots + 7) / 8 * 8;
    g.bytes = g.off_partial + (size_t)(L + 1) * g.chunks * OC_WORDS * sizeof(double);
    return g;
}

__global__ void __launch_bounds__(OC_BLOCK) level_outcomes_scan_kernel(
        uint32_t T, uint32_t n, const float* __restrict__ rew, const float* __restrict__ cost,
        const uint8_t* __restrict__ done, const uint8_t* __restrict__ trunc, const float* __restrict__ level,
        const float* __restrict__ level_values, uint32_t L, float* __restrict__ carry_ret,
        float* __restrict__ carry_cost, int32_t* __restrict__ carry_len, int32_t* __restrict__ episodes_left,
        float* __restrict__ rec_ret, float* __restrict__ rec_cost, int32_t* __restrict__ rec_len,
        uint8_t* __restrict__ tag) {
    __shared__ uint32_t s_lv[CF2_NUM_LEVELS_MAX];
    if (threadIdx.x < L) s_lv[threadIdx.x] = __float_as_uint(level_values[threadIdx.x]);
    __syncthreads();
    const uint32_t e = blockIdx.x * OC_BLOCK + threadIdx.x;
    const bool live = e < n;
    const uint32_t ec = live ? e : n - 1;             // idle lanes read a valid column and write nothing
    float er = carry_ret[ec], ecst = carry_cost[ec];
    int32_t el = carry_len[ec];
    int32_t left = episodes_left ? episodes_left[ec] : 1;
    // the scan is serial in t; the loads of U steps are issued together (as episode_stats_kernel does)
    constexpr uint32_t U = 8;
    for (uint32_t t0 = 0; t0 < T; t0 += U) {
        float rr[U], cc[U];
        uint32_t lv[U];
        uint8_t dd[U], tt[U];
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            const uint32_t t = t0 + j < T ? t0 + j : T - 1;
            const size_t k = (size_t)t * n + ec;
            rr[j] = rew[k];
            cc[j] = cost ? cost[k] : 0.0f;
            dd[j] = done[k];
            tt[j] = trunc ? trunc[k] : (uint8_t)0;
            lv[j] = level ? __float_as_uint(level[k]) : 0u;
        }
        __builtin_amdgcn_sched_barrier(0);      // the loads stay ahead of the scan
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            if (t0 + j >= T) break;
            er += rr[j];
            ecst += cc[j];
            ++el;
            uint32_t g = OC_NONE;
            const size_t k = (size_t)(t0 + j) * n + ec;
            if (dd[j] != 0) {
                if (left > 0) {
                    uint32_t bin = 0;
                    if (level) {
                        bin = L;                                     // "other": no table entry has these bits
                        for (uint32_t q = L; q-- > 0;)
                            if (s_lv[q] == lv[j]) bin = q;           // the first match
                    }
                    g = bin;
                    if (trunc) g |= tt[j] != 0 ? OC_TIMEOUT : OC_CRASH;
                    if (live) {
                        rec_ret[k] = er;
                        rec_cost[k] = ecst;
                        rec_len[k] = el;
                    }
                    if (episodes_left) --left;
                }
                er = 0.0f;
                ecst = 0.0f;
                el = 0;
            }
            if (live) tag[k] = (uint8_t)g;
        }
    }
    if (live) {
        carry_ret[e] = er;
        carry_cost[e] = ecst;
        carry_len[e] = el;
        if (episodes_left) episodes_left[e] = left;
    }
}

// one block per chunk.  Per round of OC_SPAN slots: thread i holds the tag word of slots 4 i .. 4 i + 3,
// the recorded episodes are compacted in slot order into the LDS list, and lane b < bins adds those
// of bin b.  The tag words of OC_UNROLL rounds are loaded together.
__global__ void __launch_bounds__(OC_BLOCK) level_outcomes_reduce_kernel(
        uint64_t slots, uint64_t per_chunk, uint32_t chunks, uint32_t bins, const float* __restrict__ rec_ret,
        const float* __restrict__ rec_cost, const int32_t* __restrict__ rec_len, const uint8_t* __restrict__ tag,
        double* __restrict__ partial) {
    __shared__ float l_ret[OC_SPAN], l_cost[OC_SPAN];
    __shared__ int32_t l_len[OC_SPAN];
    __shared__ uint8_t l_tag[OC_SPAN];
    __shared__ uint32_t s_wave[OC_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t begin = (uint64_t)blockIdx.x * per_chunk;
    const uint64_t end = begin + per_chunk < slots ? begin + per_chunk : slots;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(tag);
    OcAcc acc;
    acc.clear();
    for (uint64_t g0 = begin; g0 < end; g0 += OC_SPAN * OC_UNROLL) {
        uint32_t w[OC_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < OC_UNROLL; ++u) {
            const uint64_t s = g0 + (uint64_t)u * OC_SPAN + (uint64_t)tid * OC_TAGS;
            w[u] = s < end ? words[s >> 2] : 0xFFFFFFFFu;           // the word holding slots s .. s + 3
        }
#pragma unroll
        for (uint32_t u = 0; u < OC_UNROLL; ++u) {
            const uint64_t r0 = g0 + (uint64_t)u * OC_SPAN;          // block-uniform
            if (r0 >= end) break;
            const uint64_t s = r0 + (uint64_t)tid * OC_TAGS;
            // bytes past the last slot (the tag array's padding) are never written: not episodes
            uint32_t cnt = 0;
#pragma unroll
            for (uint32_t j = 0; j < OC_TAGS; ++j)
                cnt += (((w[u] >> (8u * j)) & 0xFFu) != OC_NONE && s + j < end) ? 1u : 0u;
            uint32_t incl = cnt;                                     // inclusive scan over the wave, lane order
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(incl, d);
                if ((int)lane >= d) incl += y;
            }
            if (lane == 63u) s_wave[wave] = incl;
            __syncthreads();
            uint32_t at = incl - cnt, total = 0;
#pragma unroll
            for (uint32_t v = 0; v < OC_BLOCK / 64; ++v) {
                const uint32_t c = s_wave[v];
                if (v < wave) at += c;
                total += c;
            }
#pragma unroll
            for (uint32_t j = 0; j < OC_TAGS; ++j) {
                const uint32_t g = (w[u] >> (8u * j)) & 0xFFu;
                if (g == OC_NONE || s + j >= end) continue;
                l_ret[at] = rec_ret[s + j];                          // at < total <= OC_SPAN
                l_cost[at] = rec_cost[s + j];
                l_len[at] = rec_len[s + j];
                l_tag[at] = (uint8_t)g;
                ++at;
            }
            __syncthreads();
            if (tid < bins) {
                for (uint32_t i = 0; i < total; ++i) {
                    const uint32_t g = l_tag[i];
                    if ((g & OC_BIN) != tid) continue;
                    acc.count += 1.0;
                    acc.crashes += (g & OC_CRASH) ? 1.0 : 0.0;
                    acc.timeouts += (g & OC_TIMEOUT) ? 1.0 : 0.0;
                    acc.ret.add((double)l_ret[i]);
                    acc.len.add((double)l_len[i]);
                    acc.cost.add((double)l_cost[i]);
                }
            }
            __syncthreads();                                         // the list is free for the next round
        }
    }
    if (tid < bins) acc.store(partial + ((size_t)tid * chunks + blockIdx.x) * OC_WORDS);
}

// one block per bin: thread i merges the bin's partials i, i + 256, ... in that order, then the
// block reduction
__global__ void __launch_bounds__(OC_BLOCK) level_outcomes_finalize_kernel(const double* __restrict__ partial,
                                                                           uint32_t chunks, int accumulate,
                                                                           double* __restrict__ table) {
    __shared__ double lds[(OC_BLOCK / 64) * OC_WORDS];
    const double* mine = partial + (size_t)blockIdx.x * chunks * OC_WORDS;
    double* row = table + (size_t)blockIdx.x * OC_WORDS;
    OcAcc acc;
    acc.clear();
    for (uint32_t b = threadIdx.x; b < chunks; b += OC_BLOCK) {
        OcAcc o;
        o.load(mine + (size_t)b * OC_WORDS);
        acc.merge(o);
    }
    oc_block_reduce(acc, lds);
    if (threadIdx.x == 0) {
        if (accumulate && row[0] > 0.0) {           // a row with count 0 is empty whatever it holds
            OcAcc old;
            old.load(row);
            old.merge(acc);
            acc = old;
        }
        if (!(acc.count > 0.0)) acc.clear();
        acc.store(row);
    }
}

}  // namespace cf2

using namespace cf2;

extern "C" size_t cf2_level_outcomes_scratch_bytes(uint32_t T, uint32_t n, uint32_t L) {
    if (T == 0 || n == 0 || L == 0 || L > CF2_NUM_LEVELS_MAX) return 0;
    return oc_geometry(T, n, L).bytes;
}

extern "C" int cf2_level_outcomes(uint32_t T, uint32_t n, const float* rew_dev, const float* cost_dev,
                                  const uint8_t* done_dev, const uint8_t* trunc_dev, const float* level_dev,
                                  const float* level_values_dev, uint32_t L, float* carry_ret_dev,
                                  float* carry_cost_dev, int32_t* carry_len_dev, int32_t* episodes_left_dev,
                                  double* table_dev, int accumulate, void* scratch_dev, void* stream) {
    if (L == 0 || L > CF2_NUM_LEVELS_MAX) return CF2_ERR_INVALID_ARG;
    if (T == 0 || n == 0) return CF2_OK;
    if (!rew_dev || !done_dev || !level_values_dev || !carry_ret_dev || !carry_cost_dev || !carry_len_dev ||
        !table_dev || !scratch_dev)
        return CF2_ERR_INVALID_ARG;
    const uintptr_t words = (uintptr_t)rew_dev | (uintptr_t)cost_dev | (uintptr_t)level_dev | (uintptr_t)level_values_dev |
                            (uintptr_t)carry_ret_dev | (uintptr_t)carry_cost_dev | (uintptr_t)carry_len_dev |
                            (uintptr_t)episodes_left_dev;
    if ((words & 3u) != 0 || (((uintptr_t)table_dev | (uintptr_t)scratch_dev) & 7u) != 0) return CF2_ERR_INVALID_ARG;
    const hipStream_t s = (hipStream_t)stream;
    const OcGeom g = oc_geometry(T, n, L);
    char* base = static_cast<char*>(scratch_dev);
    float* rec_ret = reinterpret_cast<float*>(base);
    float* rec_cost = reinterpret_cast<float*>(base + g.off_cost);
    int32_t* rec_len = reinterpret_cast<int32_t*>(base + g.off_len);
    uint8_t* tag = reinterpret_cast<uint8_t*>(base + g.off_tag);
    double* partial = reinterpret_cast<double*>(base + g.off_partial);
    hipLaunchKernelGGL(level_outcomes_scan_kernel, dim3((n + OC_BLOCK - 1) / OC_BLOCK), dim3(OC_BLOCK), 0, s, T, n,
                       rew_dev, cost_dev, done_dev, trunc_dev, level_dev, level_values_dev, L, carry_ret_dev,
                       carry_cost_dev, carry_len_dev, episodes_left_dev, rec_ret, rec_cost, rec_len, tag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(level_outcomes_reduce_kernel, dim3(g.chunks), dim3(OC_BLOCK), 0, s, g.slots, g.per_chunk,
                       g.chunks, L + 1, rec_ret, rec_cost, rec_len, tag, partial);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(level_outcomes_finalize_kernel, dim3(L + 1), dim3(OC_BLOCK), 0, s, partial, g.chunks, accumulate,
                       table_dev);
    e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}
