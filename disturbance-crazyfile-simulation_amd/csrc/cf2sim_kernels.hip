// cf2sim_kernels.hip -- fused CDNA4 (gfx950) env-step / reset kernels for the batched
// CrazyFlie hover environment.
//
// One lane = one env.  Env state is AoSoA in HBM: tiles of 64 envs (one wave), each env's 480 B
// as 30 float4 groups, group g of lane l at tile_base + g * 1024 + l * 16 (cf2sim_internal.h,
// DESIGN.md section 2), so every state access of a wave is one coalesced 1-KB dwordx4 transaction.
// A step loads the state once, runs aggregate_phy_steps physics sub-steps plus the
// observation / history / reward / done epilogue (and the auto-reset of finished envs) in
// registers, and stores the state once: the kernel is HBM-bound by construction (no MFMA:
// the work is per-env element-wise, not a contraction).
//
// What each piece restates (reference paths, phoenix_drone_simulation/ omitted):
//   apply_action            envs/agents.py:259-298, envs/control.py:94-100, envs/utils.py:130-134
//   force/torque assembly   envs/physics.py:213-250, envs/agents.py:300-337,517-533
//   rigid-body step         bullet3 3.21 btMultiBody (third party; see oracle/cf2_oracle.c header)
//   SimplePhysics           envs/physics.py:130-200
//   update_information      envs/agents.py:434-453
//   compute_observation     envs/hover_free.py:168-200, envs/sensors.py:75-134, envs/utils.py:102-105
//   compute_history         envs/base.py:305-321
//   reward / done / cost    envs/hover_free.py:124-235,449-461, envs/hover.py:102-202
//   reset + DR              envs/base.py:241-298,420-464, envs/hover_free.py:237-289
//   HJ disturbance          adversarial_generation/FasTrack_data/distur_gener.py:19-207,
//                           adversarial_generation/odp/Grid/GridProcessing.py:52-71
//
// This file holds the __global__ kernels, their block-level pieces and the host launch table.
// The device helpers are in headers by topic:
//   cf2sim_draws.h     random-word sources (Philox, reset table, rows), normals, helper_step_draws
//   cf2sim_math.h      rcp .. quat2euler
//   cf2sim_hj.h        HJ grid lookup and sign bits
//   cf2sim_state.h     Env, the AoSoA tile, load_* / store_*, write_obs*, LDS barrier and flags
//   cf2sim_dynamics.h  apply_action, bullet_substep, simple_substep, downwash, formation_offset
//   cf2sim_sensing.h   sensor model, observation, history, done / reward / cost, boltzmann_index
//   cf2sim_kernarg.h   late_*: kernel parameters re-read from the kernarg segment
//   cf2sim_timing.h    TSTAMP / TREADY (-DCF2_TIMING)
//   cf2sim_reset.h     reset_*, ResetSeed, reset_one, store_reset_*, reset_role
//   cf2sim_step.h      shape_view, step_env_body, step_env
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf2sim_internal.h"
#include "cf2sim_rng.h"
#include "cf2sim_policy.h"
#include "cf2sim_draws.h"
#include "cf2sim_math.h"
#include "cf2sim_hj.h"
#include "cf2sim_state.h"
#include "cf2sim_dynamics.h"
#include "cf2sim_sensing.h"
#include "cf2sim_kernarg.h"
#include "cf2sim_timing.h"
#include "cf2sim_reset.h"
#include "cf2sim_step.h"

namespace cf2 {

// ------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------
// End of a block's env-step: list the finished envs (wave ballots into per-wave lists), reset
// them block-cooperatively (see step_kernel) and write the block's obs rows out coalesced.  Every
// thread of the block calls it.
// ST_AUX, OBS_AUX: cache policy of the resets' state stores and of the obs write-out (AUX_*).
template <bool NOISE, bool DR, int PHYS, uint32_t B, uint32_t C, int TAB = 0, int ST_AUX = 0, int OBS_AUX = (int)AUX_NT>
__device__ __forceinline__ void block_epilogue(const KParams& P, const StepIO& io, uint32_t base, uint32_t tid,
                                               bool do_reset, const ResetSeed& rs, float* s_obs, uint32_t* s_list,
                                               uint32_t* s_rand, uint32_t* s_wcnt) {
    constexpr int OD = NOISE ? 34 : 42;
    constexpr uint32_t W = B / 64u;
    if (P.auto_reset) {
        // finished envs listed per wave (ballot; no atomics, no counter to initialise): wave w's
        // resets at s_list[64 w ..], its count in s_wcnt[w]; global reset order is wave-major
        const uint64_t m = __ballot(do_reset);
        const uint32_t wv = tid >> 6, lane = tid & 63u;
        if (lane == 0) s_wcnt[wv] = (uint32_t)__popcll(m);
        if (do_reset) {
            s_list[64u * wv + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = tid;
            // the seed is parked in the env's own LDS obs row (its final obs is already in
            // final_obs; the row is overwritten by the reset observation after the seed is read)
            uint32_t* row = reinterpret_cast<uint32_t*>(s_obs + tid * OD);
#pragma unroll
            for (int k = 0; k < 3; ++k) { row[k] = __float_as_uint(rs.wb[k]); row[3 + k] = __float_as_uint(rs.bias[k]); }
#pragma unroll
            for (int k = 0; k < 4; ++k) row[6 + k] = __float_as_uint(rs.ou[k]);
            row[10] = __float_as_uint(rs.level);
            row[11] = (uint32_t)rs.level_idx;
            row[SEED_CTR] = rs.ctr;
        }
        __syncthreads();
        TSTAMP(4);   // block barrier passed
        uint32_t wc[W], cnt = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; ++w) { wc[w] = s_wcnt[w]; cnt += wc[w]; }
        // global reset position -> block-local env index
        auto env_at = [&](uint32_t p) -> uint32_t {
            uint32_t w = 0;
#pragma unroll
            for (uint32_t k = 0; k + 1 < W; ++k)
                if (w == k && p >= wc[k]) { p -= wc[k]; w = k + 1; }
            return s_list[64u * w + p];
        };
        // Resets run in chunks of C envs.  Their ~26 Philox blocks per env are drawn by every
        // thread of the block in parallel into LDS; then the reset math runs on the table, split
        // by role over the four waves.  (On one lane each, the draws made the reset tail, which
        // every wave of the block waits for, about as long as the env-step itself; one wave running
        // whole resets instead of the role split: 41.2 vs 40.1 us at 262 144 envs.)
        static_assert(B == 256u, "four waves, one reset role each");
        for (uint32_t c0 = 0; c0 < cnt; c0 += C) {
            const uint32_t nc = cnt - c0 < C ? cnt - c0 : C;
            // role lanes take their seed now: this chunk's rows are only overwritten after the
            // barrier below (and other chunks' roles never touch them), so no extra barrier
            const uint32_t rl = tid & 63u, role = ((tid >> 6) + blockIdx.x) & 3u;
            const bool act = rl < nc;
            ResetSeed q;
            uint32_t t = 0;
            if (act) {
                t = env_at(c0 + rl);
                const uint32_t* row = reinterpret_cast<const uint32_t*>(s_obs + t * OD);
#pragma unroll
                for (int c = 0; c < 3; ++c) { q.wb[c] = __uint_as_float(row[c]); q.bias[c] = __uint_as_float(row[3 + c]); }
#pragma unroll
                for (int c = 0; c < 4; ++c) q.ou[c] = __uint_as_float(row[6 + c]);
                q.level = __uint_as_float(row[10]);
                q.level_idx = (int)row[11];
                q.ctr = row[SEED_CTR];
            }
            draw_reset_table<B, C>(P, base, tid, nc, s_rand, [&](uint32_t e, uint32_t& ctr, uint32_t& te) {
                te = env_at(c0 + e);
                ctr = reinterpret_cast<const uint32_t*>(s_obs + te * OD)[SEED_CTR];
            });
            __syncthreads();
            // the four waves split each reset by role (reset_role); the role of a wave rotates
            // with the block index so the co-resident blocks' roles spread over the SIMDs
            if (act) {
                const TableRng tg{s_rand + rl, C};
                reset_role<NOISE, DR, PHYS, TAB, ST_AUX>(P, io.sf, base + t, q, tg, s_obs + t * OD, role);
            }
            __syncthreads();     // the next chunk reuses s_rand
        }
        TSTAMP(12);  // every reset chunk done
    } else {
        __syncthreads();         // every obs row of the block is in LDS
    }
    write_obs_rows<B, OD, B, OBS_AUX>(io.obs + (size_t)base * OD, s_obs, P.N - base < B ? P.N - base : B, tid);
}

// The delta exchange's pack fused into the large-N env-step (cf2_step_packed above 32 768 envs):
// after block_epilogue the block's 256 rows are final in s_obs (reset rows hold the reset
// observation), so every thread writes its share of the block's o_k run, and each wave (one 64-env
// pack block) its two bitmap words, its block-table word and its resets' side entries.
template <uint32_t OL, uint32_t OD, uint32_t B>
__device__ __forceinline__ void pack_epilogue_block(const PackIO& X, uint32_t n, uint32_t base, uint32_t tid,
                                                    bool do_reset, const float* s_obs) {
    typedef float f4x __attribute__((ext_vector_type(4)));
    const PackLayout L{n, OL, X.cap};
    uint32_t* pk = X.pk;
    const uint32_t lane = tid & 63u, wbase = base + (tid & ~63u);
    const uint64_t m = __ballot(do_reset);
    uint32_t first = 0u;
    if (lane == 0 && m) first = pack_alloc(L, X.scratch, (uint32_t)__popcll(m));
    const uint32_t nvalid = n - base < B ? n - base : B;
    float* dst = reinterpret_cast<float*>(pk + L.o_slab()) + (size_t)base * OL;
    if (nvalid == B && ((uintptr_t)dst & 15u) == 0) {
        f4x* d4 = reinterpret_cast<f4x*>(dst);
        for (uint32_t c = tid; c < B * OL / 4u; c += B) {
            f4x v;
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e) {
                const uint32_t f = 4u * c + e, r = f / OL;
                v[e] = s_obs[r * OD + OL + 4u + (f - r * OL)];
            }
            d4[c] = v;
        }
    } else {
        for (uint32_t f = tid; f < nvalid * OL; f += B) {
            const uint32_t r = f / OL;
            dst[f] = s_obs[r * OD + OL + 4u + (f - r * OL)];
        }
    }
    if (wbase < n) {
        uint32_t* bits = pk + L.bits();
        if (lane == 0) bits[wbase / 32u] = (uint32_t)m;
        if (lane == 1 && wbase + 32u < n) bits[wbase / 32u + 1u] = (uint32_t)(m >> 32);
        first = __shfl(first, 0);
        if (lane == 0) pk[L.btab() + wbase / XB_PACK] = first;
        const uint32_t slot =
            pack_entry_slot(L, wbase / XB_PACK, (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), first);
        if (do_reset && slot != PACK_DROPPED) {
            uint32_t* e = pk + L.side() + slot * L.entry();
            e[0] = base + tid;
            const float* row = s_obs + tid * OD;
            float* ef = reinterpret_cast<float*>(e + 1);
#pragma unroll
            for (uint32_t k = 0; k < OL + 4u; ++k) ef[k] = row[k];     // o_0 and A (= A_0)
        }
    }
}

// Launch shape of the large-N env kernels: 256-thread blocks of 256 envs (= the auto-reset
// compaction group), 3 waves per SIMD (<= 168 VGPRs, <= 53 KB LDS per block); resets drawn and run
// in chunks of 32
constexpr uint32_t STEP_BLOCK = 256, STEP_MIN_WAVES = 3, RESET_CHUNK = 32;
// the parts of a packed store policy (store_policy_pack, cf2sim_internal.h)
constexpr int pol_state(int pol) { return pol & 0xff; }
constexpr int pol_obs(int pol) { return (pol >> 8) & 0xff; }
// Step kernel: one lane per env.  Auto-reset is compacted per block: with random actions a few
// % of envs finish per step, so nearly every wave would hold one and run the whole reset path
// divergently.  Finished envs are listed in LDS and reset by the fewest waves after a block
// barrier; their state rows were just written by this block and are still in L2, so the reset's
// scattered SoA accesses cost no extra HBM traffic (a separate reset kernel pays ~60 B per
// 4-byte field access for them).
// POL: the cache policy of its stores (store_policy_pack: state | obs rows | per-env outputs), a
// compile-time value per instance; the host picks the instance (launch_step_t).
template <bool NOISE, bool DR, int PHYS, int SPEC, int POL = (int)POL_DEFAULT>
__global__ void __launch_bounds__(STEP_BLOCK, STEP_MIN_WAVES) step_kernel(KParams P0, StepIO io, PackIO X) {
    const KParams P = shape_view<SPEC>(P0);
    // Issue priority: the blocks that start only after the first residency round (the partial
    // last round at 262 144 envs) run mostly alone on their SIMDs and end the kernel; their waves
    // get the issue slots first, so they overlap the tail of the first round (-1 us measured;
    // starting the first round's co-resident blocks 2k-8k cycles apart instead: equal or slower).
    if (blockIdx.x >= P0.late_block) __builtin_amdgcn_s_setprio(3);
    else __builtin_amdgcn_s_setprio(1);
    timing_begin();
    constexpr int OD = NOISE ? 34 : 42;
    constexpr uint32_t B = STEP_BLOCK, C = RESET_CHUNK;
    __shared__ __align__(16) float s_obs[B * OD];          // the block's obs rows, global layout
    __shared__ uint32_t s_list[B];                         // queue: block-local env index
    __shared__ uint32_t s_rand[RESET_SLOTS * 4 * C];       // the chunk's Philox blocks, [slot][word][env]
    __shared__ uint32_t s_wcnt[B / 64];                    // finished envs per wave
    const uint32_t tid = threadIdx.x, base = blockIdx.x * B, i = base + tid;
    bool do_reset = false;
    ResetSeed rs;
    __shared__ double s_hjgrid[6 * HJ_PTS];
    if (P.dstb_mode == DSTB_HJ_T) stage_hj_grid(P.tab->hj_grid, s_hjgrid);     // uniform branch
    if (i < P.N)
        do_reset = step_env<NOISE, DR, PHYS, false, false, pol_state(POL), true>(P, io, i, s_obs + tid * OD, rs, s_hjgrid);
    block_epilogue<NOISE, DR, PHYS, B, C, 2, pol_state(POL), pol_obs(POL)>(P, io, base, tid, do_reset, rs, s_obs, s_list,
                                                                           s_rand, s_wcnt);
    if (X.pk) pack_epilogue_block<NOISE ? 13u : 17u, (uint32_t)OD, B>(X, P.N, base, tid, do_reset, s_obs);
    timing_end();   // resets done
}

// An obs row in LDS as the policy's input registers of row tile rt (ObsRegs, cf2sim_policy.h; the
// 34-wide row in bf16x3): lane group g holds inputs 8 g .. 8 g + 7 (k-block 0) and 32 + g (the
// fp32 k-step; clamped, zero weight past OD)
template <int OD, int CR>
__device__ __forceinline__ void obs_regs_from_lds(const float* row, int g, ObsRegs<OD, CF2_POLICY_BF16X3, CR>& X,
                                                  int rt = 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float2 v = *reinterpret_cast<const float2*>(row + 8 * g + 2 * q);
        X.x8[rt][0][2 * q] = v.x;
        X.x8[rt][0][2 * q + 1] = v.y;
    }
    X.x1[rt][0] = row[__builtin_elementwise_min(32 + g, OD - 1)];
}

// The policy's packed fragments but layer 3's, staged from global memory into LDS by the NT threads
// of a block (the tail from O_BIAS on moves down to O_L3; the waves read layer 3 from global
// memory, L1/L2-resident).  In two halves, so that the caller draws the sampling noise while the
// loads are in flight: load() issues this thread's loads, store() puts them into LDS.
template <class PK, uint32_t NT>
struct FragmentsSkipL3 {
    static constexpr uint32_t L3N = PK::O_BIAS - PK::O_L3, WORDS = PK::TOTAL - L3N;
    static constexpr uint32_t NQ4 = WORDS / 4, NQ = (NQ4 + NT - 1) / NT;
    static_assert(PK::O_L3 % 4 == 0 && PK::O_BIAS % 4 == 0 && PK::TOTAL % 4 == 0, "float4 staging");
    float4 stg[NQ];
    __device__ __forceinline__ void load(const float* w, uint32_t tid) {
        const float4* src = reinterpret_cast<const float4*>(w);
#pragma unroll
        for (uint32_t q = 0; q < NQ; ++q) {
            const uint32_t k = __builtin_elementwise_min(tid + q * NT, NQ4 - 1u);
            stg[q] = src[k < PK::O_L3 / 4 ? k : k + L3N / 4];
        }
    }
    __device__ __forceinline__ void store(float* s_mem, uint32_t tid) const {
        float4* dst = reinterpret_cast<float4*>(s_mem);
#pragma unroll
        for (uint32_t q = 0; q < NQ; ++q)
            if (tid + q * NT < NQ4) dst[tid + q * NT] = stg[q];
    }
};

// Fused collect step: step_kernel's env-step, then the actor-critic
// forward on the block's new observations, one launch per env-step of the collect loop.  It
// replaces the pair env.step (algs/iwpg/iwpg.py:380) + ac.step (:377, algs/core.py:371-395) of
// IWPGAlgorithm.roll_out as the loop runs them back to back (policy of step t+1 right after the
// env-step of step t).  With two launches the policy kernel re-reads the obs rows from memory
// and runs alone, bound by vector issue, while the env-step leaves ~70 % of the issue slots idle
// waiting on memory; here a block's policy phase runs beside the env phases
// of the blocks sharing its CU.
//   * env phase: exactly step_kernel's (same device code: the obs, rewards, flags, final obs and
//     state are bit-identical to cf2_step's);
//   * the block's 256 obs rows are still in LDS after the write-out: each wave reads its 64 rows
//     (4 row tiles) as MFMA B operands into registers, then the block's LDS is re-used for the
//     packed fragments (52.6 KB: all but layer 3's 8 KB, which the waves read from global memory,
//     L1/L2-resident), so the kernel keeps step_kernel's 3 blocks per CU (<= 53 KB each);
//   * policy phase: policy_layers / policy_emit of cf2sim_policy.h on each of the wave's 4 row
//     tiles: the same instructions as policy_kernel, so act / val / logp are bit-identical to
//     cf2_policy_forward on the same observations.
// Built for the bench workload's shape (noise on: 34-wide observations; bf16x3 products) at
// N > 32 768 (256 envs per block); other configs return hipErrorNotSupported and the caller runs
// the two launches.
// Delaying a third of the first round's blocks by 4k / 10k / 20k cycles, so that co-resident
// blocks reach their policy phases at different times, was slower at every delay (62.1 / 64.1 /
// 67.2 vs 61.1 us at 262 144 envs, profiles/r03_collect_ab.txt); two row tiles per forward call
// (two chains interleaved, 163 VGPRs) took the same time as one.
template <bool NOISE, bool DR, int PHYS, int SPEC>
__global__ void __launch_bounds__(STEP_BLOCK, STEP_MIN_WAVES) collect_kernel(KParams P0, StepIO io, PolicyIO pio) {
    static_assert(NOISE, "the fused collect kernel is built for the 34-wide observation");
    const KParams P = shape_view<SPEC>(P0);
    if (blockIdx.x >= P0.late_block) __builtin_amdgcn_s_setprio(3);
    else __builtin_amdgcn_s_setprio(1);
    constexpr int OD = 34;
    constexpr uint32_t B = STEP_BLOCK, C = RESET_CHUNK, W = B / 64u;
    static_assert(B == 256, "one 64-row wave per SIMD quarter of the block");
    using PK = Packed<OD, CF2_POLICY_BF16X3>;
    // LDS: the env phase's arrays, then the fragments but layer 3 (the tail from O_BIAS on moves
    // down to O_L3)
    using Frags = FragmentsSkipL3<PK, B>;
    constexpr uint32_t HJ_AT = (B * OD + B + RESET_SLOTS * 4 * C + W + 1) & ~1u;     // 8-B aligned
    constexpr uint32_t ENV_WORDS = HJ_AT + 2 * 6 * HJ_PTS;
    constexpr uint32_t LDS_WORDS = Frags::WORDS > ENV_WORDS ? Frags::WORDS : ENV_WORDS;
    __shared__ __align__(16) float s_mem[LDS_WORDS];
    float* s_obs = s_mem;
    uint32_t* s_list = reinterpret_cast<uint32_t*>(s_mem + B * OD);
    uint32_t* s_rand = s_list + B;
    uint32_t* s_wcnt = s_rand + RESET_SLOTS * 4 * C;
    double* s_hjgrid = reinterpret_cast<double*>(s_mem + HJ_AT);
    const uint32_t tid = threadIdx.x, base = blockIdx.x * B, i = base + tid;
    bool do_reset = false;
    ResetSeed rs;
    if (P.dstb_mode == DSTB_HJ_T) stage_hj_grid(P.tab->hj_grid, s_hjgrid);     // uniform branch
    // kernel parameters re-read where used, as step_kernel (-0.8 us per env-step of the collect loop)
    if (i < P.N) do_reset = step_env<NOISE, DR, PHYS, false, false, 0, true>(P, io, i, s_obs + tid * OD, rs, s_hjgrid);
    block_epilogue<NOISE, DR, PHYS, B, C, 2>(P, io, base, tid, do_reset, rs, s_obs, s_list, s_rand, s_wcnt);
    // ---- policy phase.  Lane l of wave wv holds, for row tile c, row 64 wv + 16 c + (l & 15):
    // inputs 8 g .. 8 g + 7 (k-block 0) and 32 + g (the fp32 k-step; clamped, zero weight past D)
    const uint32_t l = tid & 63u, wv = tid >> 6, r16 = l & 15u;
    const int g = (int)(l >> 4);
    constexpr int CR = 1, NCH = 4 / CR;                       // row tiles per forward call, calls per wave
    ObsRegs<OD, CF2_POLICY_BF16X3, CR> X[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int rt = 0; rt < CR; ++rt)
            obs_regs_from_lds(s_obs + (64u * wv + 16u * (uint32_t)(CR * c + rt) + r16) * OD, g, X[c], rt);
    __syncthreads();         // every wave holds its rows: the LDS takes the fragments
    // fragment loads first; while they are in flight each lane draws the sampling noise of the
    // wave's row 64 wv + l (one Philox block per row, instead of one per row tile on all 64 lanes)
    Frags frags;
    frags.load(pio.w, tid);
    float ep[4];
    policy_noise(pio.key0, pio.key1, pio.counter, pio.row_offset + base + 64u * wv + l, ep);
    frags.store(s_mem, tid);
    __syncthreads();
    PolicyLane<OD, CF2_POLICY_BF16X3> CL;
    policy_lane_init<OD, CF2_POLICY_BF16X3>(s_mem + PK::O_L3, g, CL);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {          // unrolled: X[c] stays in registers
        int off = 0;
        asm volatile("" : "+v"(off));        // keep the fragment reads inside the loop (policy_kernel)
        const float* sw = s_mem + off;
        ObsRegs<OD, CF2_POLICY_BF16X3, CR> Xc = X[c];
        policy_standardize<OD, CF2_POLICY_BF16X3, CR>(sw + PK::O_L3, g, CL, Xc);
        f4v o[CR];
        policy_layers<OD, CF2_POLICY_BF16X3, 0, CR>(sw, sw + PK::O_L3, pio.w + PK::O_L3, (int)l, Xc, o);
#pragma unroll
        for (int rt = 0; rt < CR; ++rt) {
            const uint32_t wr = 16u * (uint32_t)(CR * c + rt) + r16, row = base + 64u * wv + wr;
            float e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)      // row wr's noise from lane wr
                e[k] = __int_as_float(__builtin_amdgcn_ds_bpermute((int)(wr << 2), __float_as_int(ep[k])));
            if (row < P.N)
                policy_emit_eps<OD, CF2_POLICY_BF16X3, 0>(o[rt], row, g, CL, e, 1, pio.act, pio.val, pio.logp,
                                                          nullptr);
        }
    }
}

// Small N (<= 32 768 envs): the launch is as long as one wave's env-step chain, and the auto-reset
// tail used to be ~40 % of it (section 3 describes this kernel).  Each 256-thread block holds 64 envs.  Wave 0
// steps them (issue priority 3).  Waves 1-3 meanwhile compute, speculatively for all 64 envs and at
// priority 0, every part of a potential auto-reset that does not depend on the finished episode:
// a reset's draws are keyed by the env's RNG counter, which is known when the state loads, so
// they are the same Philox blocks the reset would draw after the step.
//   wave 1 (A): reset pose, velocities, motor state, latency ring    (reset_kinematics), domain
//               randomisation, disturbance, level (reset_params)
//   wave 2 (B): the pose again, the first reset sensor call's held measurement and gyro normals;
//               stages the reset observation row but for its two gyro-LPF triples
//   wave 3 (C): the pose again and the second sensor call's held part (into the staged row) and
//               gyro normals (handed to B in LDS)
// After one LDS barrier only the finished envs' work remains, on their lanes of waves 1-3: the two
// gyro updates, which need the finished episode's body rates (the gyro LPF seed) and gyro bias,
// the reset observation row, and the reset's state stores (store_reset_*).  The env wave does not
// store the state of envs that reset (step_env_body), so no group is stored twice.
// Measured and not kept: reward, cost and the per-env outputs finished by helper wave 3 from an
// LDS table after the barrier (32 768 envs 10.3 -> 11.0 us: the reset tail grew more than the env
// wave's epilogue shrank); the DR draws before the draw barrier (10.6 -> 11.2 us).
enum { SEED_SMALL = 10 };   // per finished env, wave 0 -> waves 1-3: final body rates, gyro bias, OU state
enum { C2_WORDS = 9 };      // per env, wave 3 -> wave 2: the second reset sensor call's gyro normals

// The delta exchange's pack fused into the small-N env-step (cf2_step_packed; the layout and the
// side-slot allocation are cf2sim_pack.h's, the standalone form is obs_pack_kernel): wave 2, once the
// reset rows are final (s_rrow; the other rows are final in s_obs at the block barrier), writes the
// block's bitmap words and block-table word, each lane its row's o_k (13 or 17 dword stores, the
// wave's together a contiguous run) and, for a reset row, its side entry.  The packed buffer is then
// ready for the all-gather when the env-step kernel ends: no pack kernel, no re-read of the
// observation rows.  A block with more resets than its quota asks for spill slots (pack_alloc, a
// memory-side atomic) right after the block barrier, so the atomic's round trip overlaps the reset
// tail.  The informational header words are not written and the zeroing of the counter is the
// caller's (cf2_xchg_* zeroes a batch's counters in its consume): as little as a block-0 store of
// the header in this kernel slowed even the unpacked env-step from 9.5 to 10.6-11.0 us at 32 768
// envs, and a
// word-interleaved o_k run (one coalesced store per 64 words, ~1000 more instructions) did the same
// (tools/pack_cost_probe.py with ablation builds, gpurun_out/r05r-r05x): the small kernel's env wave
// is sensitive to code anywhere in the kernel.
template <uint32_t OL, uint32_t OD>
__device__ __forceinline__ void pack_epilogue(const PackIO& X, uint32_t n, uint32_t base, uint32_t nvalid,
                                              uint64_t mask, const float* s_obs, const float* s_rrow, uint32_t lane,
                                              uint32_t first) {
    const PackLayout L{n, OL, X.cap};
    uint32_t* pk = X.pk;
    uint32_t* bits = pk + L.bits();
    if (lane == 0) bits[base / 32u] = (uint32_t)mask;
    if (lane == 1 && base + 32u < n) bits[base / 32u + 1u] = (uint32_t)(mask >> 32);
    first = __shfl(first, 0);          // lane 0's pack_alloc, issued right after the block barrier
    if (lane == 0) pk[L.btab() + base / XB_PACK] = first;
    if (lane >= nvalid) return;
    const bool rs = (mask >> lane) & 1ull;
    const float* row = (rs ? s_rrow : s_obs) + lane * OD;
    float* ok = reinterpret_cast<float*>(pk + L.o_slab()) + (size_t)(base + lane) * OL;
#pragma unroll
    for (uint32_t k = 0; k < OL; ++k) ok[k] = row[OL + 4u + k];
    if (!rs) return;
    const uint32_t slot = pack_entry_slot(L, base / XB_PACK, (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), first);
    if (slot == PACK_DROPPED) return;
    uint32_t* e = pk + L.side() + slot * L.entry();
    e[0] = base + lane;
    float* ef = reinterpret_cast<float*>(e + 1);
#pragma unroll
    for (uint32_t k = 0; k < OL + 4u; ++k) ef[k] = row[k];     // o_0 and A (= A_0)
}

// The small-N kernel's LDS arrays (step_kernel_small declares them; collect_kernel_small carves
// them out of a buffer the policy fragments re-use afterwards)
template <bool NOISE, int SPEC>
struct SmallLds {
    static constexpr int OL = NOISE ? 13 : 17, OD = 2 * (OL + 4);
    // reference-default shape with sensor noise: the helpers also draw the env-step's randomness
    // after its first sub-step (HD_* layout), handed over at an LDS barrier before sub-step 1
    static constexpr bool HD = SPEC == 1 && NOISE;
    // word offsets in a carved buffer (doubles 8-B aligned, rows 16-B aligned)
    // (HD: wave 1 computes the reset pose once and hands it to waves 2-3: POSE_WORDS per env behind
    // the flag word s_mask[2])
    static constexpr uint32_t POSE_WORDS = HD ? 12 : 0;
    static constexpr uint32_t O_OBS = 0, O_RROW = 64 * OD, O_SEED = 128 * OD, O_C2 = O_SEED + SEED_SMALL * 64,
                              O_DRAW = O_C2 + C2_WORDS * 64, O_POSE = O_DRAW + (HD ? HD_WORDS * 64 : 1),
                              O_MASK = O_POSE + (HD ? POSE_WORDS * 64 : 1),
                              O_HJ = (O_MASK + 3 + 1) & ~1u, WORDS = O_HJ + 2 * 6 * HJ_PTS;
};

template <bool NOISE, bool DR, int PHYS, int SPEC>
__device__ __forceinline__ uint64_t small_body(const KParams& P0, const StepIO& io, float* s_obs, float* s_seed,
                                               float* s_c2, float* s_rrow, uint32_t* s_mask, double* s_hjgrid,
                                               float* s_draw, float* s_pose, const PackIO& X = PackIO{}) {
    const KParams P = shape_view<SPEC>(P0);
    using SL = SmallLds<NOISE, SPEC>;
    constexpr int OL = SL::OL;
    constexpr int OD = SL::OD;
    constexpr bool HD = SL::HD;
    timing_begin();
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t base = blockIdx.x * 64u, i = base + lane, gid = P.gid_off + i;
    const bool live = i < P.N;
    if (P.dstb_mode == DSTB_HJ_T) stage_hj_grid(P.tab->hj_grid, s_hjgrid);     // uniform branch
    const Tile T(io.sf, P.N, i);
    // the domain randomisation / disturbance / level draws of the reset: wave 3 (in the
    // reference-default shape wave 1 computes the reset pose for all three helpers meanwhile)
    constexpr uint32_t PARAMS_WAVE = 3u;
    Env H;                         // waves 1-3: the speculative reset (kept across the barrier)
    float held1[10], ng1[9];       // wave 2: first reset sensor call
    HeldNoise hn;                  // waves 2 / 3: the noise of the first / second reset sensor call
    float ngs[9];                  //   and its gyro normals
    uint32_t ctr = 0;
    if (wave != 0 && live) ctr = helper_counter(T);      // the env's counter (step and reset draws)
    const Keys K = make_keys(P.key0, P.key1);
    const Rng gr{K, ctr, gid, TAG_RESET};
    // the speculative reset's work that needs no reset pose: DR / disturbance / level draws (wave
    // PARAMS_WAVE) and the two reset sensor calls' noise (waves 2, 3), after the draw barrier (all
    // of it before that barrier, in the time the helpers wait there, made the env wave wait at it)
    auto reset_prework = [&]() {
        if (wave == PARAMS_WAVE) {
            helper_level(P, T, P.need_level || io.level != nullptr, H.level, H.level_idx);
            reset_params<DR>(P, H, gr);
        }
        if (NOISE && wave >= 2) held_noise(P, gr, wave == 2 ? 32u : 40u, hn, ngs);
    };
    if (HD && wave != 0) {
        // the env-step's draws after sub-step 0 (step tag, the env's counter), split over the
        // three helper waves; Box-Muller applied where the env-step turns words into normals
        if (live) helper_step_draws(K, ctr, gid, wave, s_draw + lane);
        if (wave == 1 && lane == 0) s_mask[2] = 0u;     // the pose flag (set once the pose is in LDS)
        TSTAMP(10);      // helper: step draws in LDS
        lds_barrier();   // joined by the env wave before its second sub-step (step_env_body)
        TSTAMP(11);
    }
    if (wave == 0) {
        __builtin_amdgcn_s_setprio(3);
        bool do_reset = false;
        ResetSeed rs;
        if (live)
            do_reset = step_env<NOISE, DR, PHYS, true, HD>(P, io, i, s_obs + lane * OD, rs, s_hjgrid, s_draw + lane);
        const uint64_t m = __ballot(do_reset);
        if (lane == 0) { s_mask[0] = (uint32_t)m; s_mask[1] = (uint32_t)(m >> 32); }
        if (do_reset) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { s_seed[k * 64 + lane] = rs.wb[k]; s_seed[(3 + k) * 64 + lane] = rs.bias[k]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) s_seed[(6 + k) * 64 + lane] = rs.ou[k];
        }
    } else if (HD && P.auto_reset && live) {
        // the reset pose computed once, by wave 1 (its step draws are the fewest), and handed to
        // waves 2-3 in LDS while they turn their sensor-call draws into noise (and wave 3 draws the
        // reset's parameters)
        __builtin_amdgcn_s_setprio(0);
        float* row = s_rrow + lane * OD;
        if (wave == 1) {
            reset_kinematics<PHYS>(P, H, gr, gid);
#pragma unroll
            for (int k = 0; k < 4; ++k) { row[OL + k] = H.la[k]; row[2 * OL + 4 + k] = H.la[k]; }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_pose[k * 64 + lane] = H.p[k];
                s_pose[(3 + k) * 64 + lane] = H.v[k];
                s_pose[(6 + k) * 64 + lane] = H.rpy[k];
                s_pose[(9 + k) * 64 + lane] = H.wb[k];
            }
            if (lane == 0) lds_flag_set(s_mask + 2);
        }
        reset_prework();
        if (wave >= 2) {
            lds_flag_wait(s_mask + 2, P.tab);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                H.p[k] = s_pose[k * 64 + lane];
                H.v[k] = s_pose[(3 + k) * 64 + lane];
                H.rpy[k] = s_pose[(6 + k) * 64 + lane];
                H.wb[k] = s_pose[(9 + k) * 64 + lane];
            }
            if (wave == 2) {
                held_combine(H, hn, held1);
#pragma unroll
                for (int k = 0; k < 9; ++k) ng1[k] = ngs[k];
#pragma unroll
                for (int k = 0; k < 10; ++k) row[k] = held1[k];
            } else {
                float held2[10];
                held_combine(H, hn, held2);
#pragma unroll
                for (int k = 0; k < 10; ++k) row[OL + 4 + k] = held2[k];
#pragma unroll
                for (int k = 0; k < 9; ++k) s_c2[k * 64 + lane] = ngs[k];
            }
        }
        TREADY("v"(H.p[0]), "v"(H.K[3]), "v"(H.la[3]));
        TSTAMP(9);   // helper: speculative reset computed
    } else if (!HD && P.auto_reset && live) {
        __builtin_amdgcn_s_setprio(0);
        reset_prework();
        if (wave == 1) {
            reset_kinematics<PHYS>(P, H, gr, gid);
        } else if (wave == 2) {
            reset_kinematics<PHYS>(P, H, gr, gid);
            // the reset observation row [o_0, A_0, o_1, A_1] as far as it does not depend on the
            // finished episode: all of it but the two gyro-LPF triples (o_1's held part: wave 3)
            float* row = s_rrow + lane * OD;
            if (NOISE) {
                held_combine(H, hn, held1);
#pragma unroll
                for (int k = 0; k < 9; ++k) ng1[k] = ngs[k];
#pragma unroll
                for (int k = 0; k < 10; ++k) row[k] = held1[k];
            } else {
                float o[17];
                plain_obs(H, o);
#pragma unroll
                for (int k = 0; k < 17; ++k) { row[k] = o[k]; row[OL + 4 + k] = o[k]; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) { row[OL + k] = H.la[k]; row[2 * OL + 4 + k] = H.la[k]; }
        } else if (NOISE) {
            Env H2;
            reset_kinematics<PHYS>(P, H2, gr, gid);
            float held2[10];
            held_combine(H2, hn, held2);
            float* row = s_rrow + lane * OD;
#pragma unroll
            for (int k = 0; k < 10; ++k) row[OL + 4 + k] = held2[k];
#pragma unroll
            for (int k = 0; k < 9; ++k) s_c2[k * 64 + lane] = ngs[k];
        }
        TREADY("v"(H.p[0]), "v"(H.K[3]), "v"(H.la[3]));
        TSTAMP(9);   // helper: speculative reset computed
    }
    lds_barrier();
    TSTAMP(4);   // block barrier passed
    const uint64_t mask = ((uint64_t)s_mask[1] << 32) | (uint64_t)s_mask[0];
    const bool mine = wave != 0 && ((mask >> lane) & 1ull);
    uint32_t pk_first = 0u;          // fused pack: the block's first side slot (wave 2, lane 0)
    if (X.pk && wave == 2 && lane == 0 && mask)
        pk_first = pack_alloc(PackLayout{P.N, (uint32_t)OL, X.cap}, X.scratch, (uint32_t)__popcll(mask));
    if (mine) {
        TSTAMP(6);
        if (wave == 1) {
            const float ou[4] = {s_seed[6 * 64 + lane], s_seed[7 * 64 + lane], s_seed[8 * 64 + lane], s_seed[9 * 64 + lane]};
            store_reset_kinematics<PHYS>(P, T, H, ou, ctr);
        } else if (wave == 2) {
            // the reset observation (reset_observe: two sensor calls, then the history row): the
            // gyro-LPF triples of o_0 and o_1 complete the staged row
            Env& E = H;
            float* row = s_rrow + lane * OD;
            if (HD) {
#pragma unroll
                for (int k = 0; k < 4; ++k) E.la[k] = row[OL + k];     // wave 1's, staged in the row
            }
            if (NOISE) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { E.lpf[k] = s_seed[k * 64 + lane]; E.bias[k] = s_seed[(3 + k) * 64 + lane]; }
                float ng2[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) ng2[k] = s_c2[k * 64 + lane];
#pragma unroll
                for (int k = 0; k < 10; ++k) E.held[k] = row[OL + 4 + k];
                gyro_update(P, E, ng1);
#pragma unroll
                for (int k = 0; k < 3; ++k) row[10 + k] = E.lpf[k];
                gyro_update(P, E, ng2);
#pragma unroll
                for (int k = 0; k < 3; ++k) row[OL + 4 + 10 + k] = E.lpf[k];
#pragma unroll
                for (int k = 0; k < 10; ++k) E.obs_prev[k] = E.held[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) E.obs_prev[10 + k] = E.lpf[k];
            } else {
#pragma unroll
                for (int k = 0; k < OL; ++k) E.obs_prev[k] = row[OL + 4 + k];
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int k = 0; k < 4; ++k) E.hact[s2][k] = E.la[k];
            store_reset_history<NOISE>(P, T, E);
            TSTAMP(8);
        }
        if (wave == PARAMS_WAVE) store_reset_params<DR>(P, T, H);
    }
    // the block's obs rows: the chunks of rows whose env did not reset by the env wave (done with
    // its env-step), the chunks touching a reset row by wave 2 once it has completed those rows (its
    // own LDS writes precede its reads; with sensor noise it writes the rows' gyro-LPF triples above).
    // No second barrier: the two sets are disjoint (measured against a block barrier followed by a
    // 256-thread merged write-out: see DESIGN.md section 3).
    const uint32_t nvalid = P.N - base < 64u ? P.N - base : 64u;
    if (wave == 0) write_obs_rows_part<OD>(io.obs + (size_t)base * OD, s_obs, s_rrow, mask, nvalid, lane, false);
    else if (wave == 2) {
        write_obs_rows_part<OD>(io.obs + (size_t)base * OD, s_obs, s_rrow, mask, nvalid, lane, true);
        if (X.pk) pack_epilogue<OL, OD>(X, P.N, base, nvalid, mask, s_obs, s_rrow, lane, pk_first);
    }
    TSTAMP(12);  // rows written
    timing_end();
    return mask;
}

template <bool NOISE, bool DR, int PHYS, int SPEC>
__global__ void __launch_bounds__(256, 2) step_kernel_small(KParams P0, StepIO io, PackIO X) {
    using SL = SmallLds<NOISE, SPEC>;
    __shared__ __align__(16) float s_obs[64 * SL::OD];     // the block's obs rows, global layout
    __shared__ float s_seed[SEED_SMALL * 64];              // [word][env]
    __shared__ float s_c2[C2_WORDS * 64];                  // [word][env]
    __shared__ __align__(16) float s_rrow[64 * SL::OD];    // speculative reset observation rows
    __shared__ uint32_t s_mask[3];                         // finished envs (ballot of wave 0), pose flag
    __shared__ double s_hjgrid[6 * HJ_PTS];
    __shared__ float s_draw[SL::HD ? HD_WORDS * 64 : 1];
    __shared__ float s_pose[SL::HD ? SL::POSE_WORDS * 64 : 1];
    (void)small_body<NOISE, DR, PHYS, SPEC>(P0, io, s_obs, s_seed, s_c2, s_rrow, s_mask, s_hjgrid, s_draw, s_pose, X);
}

// The fused collect step at small N (N <= 32 768: the 8-GPU node shard, C2): step_kernel_small's
// env-step (64 envs per block, helper waves), then the policy forward of the block's 64 new
// observations, one 16-row tile per wave.  Alone, the policy kernel at these sizes is a fixed
// cost (weights staging + one tile's dependent chain + a launch: ~15-18 us per step at 4096-32 768
// rows, more than the env-step); here it follows the env-step inside the block.  The final
// observation rows are read from LDS (s_obs, or s_rrow where the env reset), then the block's LDS
// takes the fragments (all but layer 3, as collect_kernel).  Outputs bit-identical to cf2_step +
// cf2_policy_forward.
template <bool NOISE, bool DR, int PHYS, int SPEC>
__global__ void __launch_bounds__(256, 2) collect_kernel_small(KParams P0, StepIO io, PolicyIO pio) {
    static_assert(NOISE, "the fused collect kernel is built for the 34-wide observation");
    using SL = SmallLds<NOISE, SPEC>;
    constexpr int OD = SL::OD;
    using PK = Packed<OD, CF2_POLICY_BF16X3>;
    using Frags = FragmentsSkipL3<PK, 256u>;
    constexpr uint32_t LDS_WORDS = Frags::WORDS > SL::WORDS ? Frags::WORDS : SL::WORDS;
    __shared__ __align__(16) float s_mem[LDS_WORDS];
    const uint64_t mask = small_body<NOISE, DR, PHYS, SPEC>(
        P0, io, s_mem + SL::O_OBS, s_mem + SL::O_SEED, s_mem + SL::O_C2, s_mem + SL::O_RROW,
        reinterpret_cast<uint32_t*>(s_mem + SL::O_MASK), reinterpret_cast<double*>(s_mem + SL::O_HJ),
        s_mem + SL::O_DRAW, s_mem + SL::O_POSE);
    // ---- policy phase: wave w takes rows 16 w .. 16 w + 15 of the block (lane l: row 16 w + (l & 15),
    // inputs 8 g .. 8 g + 7 and 32 + g), once wave 2 has completed the reset rows
    lds_barrier();
    const uint32_t tid = threadIdx.x, l = tid & 63u, wv = tid >> 6, r16 = l & 15u;
    const int g = (int)(l >> 4);
    const uint32_t br = 16u * wv + r16, base = blockIdx.x * 64u, row = base + br;
    ObsRegs<OD, CF2_POLICY_BF16X3> X;
    obs_regs_from_lds((((mask >> br) & 1ull) ? s_mem + SL::O_RROW : s_mem + SL::O_OBS) + br * OD, g, X);
    __syncthreads();         // every wave holds its rows: the LDS takes the fragments
    Frags frags;
    frags.load(pio.w, tid);
    float ep[4];             // this lane's row's sampling noise, drawn while the loads are in flight
    policy_noise(pio.key0, pio.key1, pio.counter, pio.row_offset + row, ep);
    frags.store(s_mem, tid);
    __syncthreads();
    PolicyLane<OD, CF2_POLICY_BF16X3> CL;
    policy_lane_init<OD, CF2_POLICY_BF16X3>(s_mem + PK::O_L3, g, CL);
    policy_standardize<OD, CF2_POLICY_BF16X3>(s_mem + PK::O_L3, g, CL, X);
    f4v o[1];
    policy_layers<OD, CF2_POLICY_BF16X3, 0>(s_mem, s_mem + PK::O_L3, pio.w + PK::O_L3, (int)l, X, o);
    if (row < P0.N)
        policy_emit_eps<OD, CF2_POLICY_BF16X3, 0>(o[0], row, g, CL, ep, 1, pio.act, pio.val, pio.logp, nullptr);
}

// One physics sub-step of every env: the physics plugin's step_forward on its own (PyBulletPhysics
// physics.py:91-124, SimplePhysics :130-200, PybulletPhysicsWithAdversary :213-250): apply_action,
// force/torque assembly, drag, rigid-body step and readback; no observation, reward or episode
// counter (cf2_physics_step).  OU normals: Philox block 0 of (rng counter, TAG_PHYS).
template <bool NOISE, bool DR, int PHYS>
__global__ void __launch_bounds__(256) physics_kernel(KParams P, float* __restrict__ sf, const float* __restrict__ act,
                                                      const float* __restrict__ dstb, float dt_override) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.N) return;
    Env E;
    load_env<NOISE, DR, PHYS>(P, sf, i, E, false, /*with_hist=*/false);
    // one sub-step leaves the ring's rows unequal: a compact env goes back to explicit rows (store_core
    // writes all of them, the flag word below has the bit clear) and its hact[1], ring row 0 as loaded,
    // is materialised in G_HACT + 1
    const F4 row0 = f4(E.abuf[0][0], E.abuf[0][1], E.abuf[0][2], E.abuf[0][3]);
    const float4 a4 = reinterpret_cast<const float4*>(act)[i];
    const float a[4] = {a4.x, a4.y, a4.z, a4.w};
    float d[3] = {0.0f, 0.0f, 0.0f};
    if (dstb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = dstb[(size_t)i * 3 + k];
    }
    if (dt_override > 0.0f) E.dt = dt_override;
    const Keys K = make_keys(P.key0, P.key1);
    const Rng g{K, E.rng, P.gid_off + i, TAG_PHYS};
    float on[4];
    normals<4>(g, 0, on);
    if (PHYS == PHYS_BULLET_T) {
        if (P.ground_effect) {
            euler_from_quat(E.q, E.rpy);     // drone.rpy of the last readback
            bullet_substep<true>(P, E, a, d, on, E.ep_step == 0 && !E.props_on);
        } else {
            bullet_substep<false>(P, E, a, d, on, E.ep_step == 0 && !E.props_on);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) E.wb[k] = E.w[k];
        simple_substep(P, E, a, on);
    }
    E.props_on = 1;
    E.rng += 1;
    store_core<NOISE, DR, PHYS>(P, sf, i, E);
    const Tile T(sf, P.N, i);
    if (E.compact) T.st(G_HACT + 1, row0);
    const int fl = (E.aidx & 15) | (E.halias0 << 4) | (E.halias1 << 5) | (E.la_view << 6) | (E.props_on << 7);
    T.st(G_CORE3, f4(E.w[2], ib(E.ep_step), ib((int)E.rng), ib(fl)));
}

// Step k's view of a K-step launch's StepIO: the k-th [n, ...] slab of every per-env output (n rows
// per slab, the whole population; od floats per observation row).  act: step k's actions, which
// the callers find differently (the rollout strides its action tensor, the collect loop reads the
// policy's slab k).  obs stays the caller's: the kernels write a block's rows from LDS, and reading
// the slab's base through this view cost the fused rollout registers (its benchmark instance
// 36 -> 68 B of scratch).
__host__ __device__ __forceinline__ StepIO step_slab(const StepIO& io, const float* act, size_t k, size_t n, size_t od) {
    StepIO s = io;
    s.act = act;
    s.rew = io.rew + k * n;
    s.done = io.done + k * n;
    if (io.trunc) s.trunc = io.trunc + k * n;
    if (io.cost) s.cost = io.cost + k * n;
    if (io.level) s.level = io.level + k * n;
    if (io.final_obs) s.final_obs = io.final_obs + k * n * od;
    return s;
}

// The fused rollout's auto-resets (rollout_kernel): the block lists its
// finished envs, draws their reset tables block-parallel as step_kernel does, and each env is
// then reset in place by its own lane (its state is in that lane's registers); the reset
// observation goes to row (this lane's LDS row or its global obs row).  Begins and ends with a
// block barrier; s_cnt was zeroed before the first one.
template <bool NOISE, bool DR, int PHYS, uint32_t B, uint32_t C>
__device__ __forceinline__ void rollout_resets(const KParams& P, Env& E, uint32_t base, uint32_t tid, uint32_t i,
                                               bool do_reset, const ResetSeed& rs, uint32_t* s_cnt,
                                               uint32_t* s_list, uint32_t* s_ctr, uint32_t* s_rand, float* row) {
    constexpr int OD = NOISE ? 34 : 42;
    __syncthreads();             // s_cnt initialised
    uint32_t pos = 0;
    const uint64_t m = __ballot(do_reset);
    if (m) {
        const int lane = (int)(threadIdx.x & 63);
        const int leader = __ffsll((unsigned long long)m) - 1;
        if (lane == leader) pos = atomicAdd(s_cnt, (uint32_t)__popcll(m));
        pos = __shfl(pos, leader) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (do_reset) { s_list[pos] = tid; s_ctr[pos] = rs.ctr; }
    }
    __syncthreads();
    const uint32_t cnt = *s_cnt;
    for (uint32_t c0 = 0; c0 < cnt; c0 += C) {
        const uint32_t nc = cnt - c0 < C ? cnt - c0 : C;
        draw_reset_table<B, C>(P, base, tid, nc, s_rand, [&](uint32_t e, uint32_t& ctr, uint32_t& te) {
            ctr = s_ctr[c0 + e];
            te = s_list[c0 + e];
        });
        __syncthreads();
        if (do_reset && pos >= c0 && pos < c0 + nc) {
            // reset_env keeps what a reset inherits from the finished episode (stale body rates,
            // gyro bias, OU state, level) from E itself
            float o[OD];
            const TableRng tg{s_rand + (pos - c0), C};
            reset_env<NOISE, DR, PHYS, /*TAB=*/true>(P, E, tg, P.gid_off + i, o);
#pragma unroll
            for (int q = 0; q < OD; q += 2) *reinterpret_cast<float2*>(row + q) = make_float2(o[q], o[q + 1]);
        }
        __syncthreads();         // the next chunk reuses s_rand
    }
}

// Fused K-step rollout (cf2_rollout): the env state is loaded once, stays in registers for K
// env-steps and is stored once.  Step k reads its actions at act + k * act_stride and writes its
// outputs into the k-th [N, ...] slab of each output (obs, rew, done, trunc, cost, level,
// final_obs), i.e. exactly what K cf2_step calls would write.  Auto-reset: the block lists its
// finished envs and draws their reset tables block-parallel as step_kernel does, but each env is
// then reset in place by its own lane (its state is in that lane's registers); per env-step HBM
// traffic is the actions and the outputs only (~170 B instead of ~765 B).
// 2 waves per SIMD: the whole state stays live across the loop (~270 registers at peak).  The 20
// Philox round keys in SGPRs make it spill 28 B/lane of VGPRs (7 registers); re-deriving them per
// Philox call removes every VGPR spill but was slower on MI355X (K = 32 per env-step: 27.9 -> 30.0
// us at 262 144 envs, 8.5 -> 10.1 us at 4096): the SALU adds sit in each Philox chain, the spills
// do not.
constexpr uint32_t ROLL_MIN_WAVES = 2;
template <bool NOISE, bool DR, int PHYS, int SPEC>
__global__ void __launch_bounds__(STEP_BLOCK, ROLL_MIN_WAVES) rollout_kernel(KParams P0, StepIO io0, uint32_t K,
                                                                          uint32_t act_stride) {
    const KParams P = shape_view<SPEC>(P0);
    constexpr int OD = NOISE ? 34 : 42;
    constexpr uint32_t B = STEP_BLOCK, EPB = STEP_BLOCK;
    constexpr uint32_t C = RESET_CHUNK;
    __shared__ __align__(16) float s_obs[B * OD];
    __shared__ uint32_t s_list[B];
    __shared__ uint32_t s_ctr[B];                       // rng counter of each listed env's reset
    __shared__ uint32_t s_rand[RESET_SLOTS * 4 * C];
    __shared__ uint32_t s_cnt;
    __shared__ double s_hjgrid[6 * HJ_PTS];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * EPB, i = base + tid;
    if (P.dstb_mode == DSTB_HJ_T) stage_hj_grid(P.tab->hj_grid, s_hjgrid);     // uniform branch
    const bool live = tid < EPB && i < P.N;
    const bool need_level = P.need_level || io0.level != nullptr;
    Env E;
    if (live) load_env<NOISE, DR, PHYS>(P, io0.sf, i, E, need_level, /*with_hist=*/true);
    const size_t n = P0.out_stride;              // rows per output slab (the whole population)
    float* obs_row = s_obs + tid * OD;
    for (uint32_t k = 0; k < K; ++k) {
        if (tid == 0) s_cnt = 0;     // every reader of the previous step passed its last barrier
        const StepIO I0 = late_io(io0);
        const StepIO io = step_slab(I0, I0.act + (size_t)k * act_stride, k, n, OD);
        bool do_reset = false;
        ResetSeed rs;
        if (live) do_reset = step_env_body<NOISE, DR, PHYS, false, false, false, 0, false, true>(P, io, i, E, obs_row, rs, s_hjgrid);
        rollout_resets<NOISE, DR, PHYS, B, C>(P, E, base, tid, i, do_reset, rs, &s_cnt, s_list, s_ctr, s_rand, obs_row);
        // coalesced write of the block's obs rows into step k's slab
        write_obs_rows<EPB, OD, B>(io0.obs + (size_t)k * n * OD + (size_t)base * OD, s_obs,
                                   P.N - base < EPB ? P.N - base : EPB, tid);
        __syncthreads();             // the write-out read s_obs before the next step's rows
    }
    if (live) store_env<NOISE, DR, PHYS>(P, io0.sf, i, E, /*params_dirty=*/true);
}

// Small-N fused rollout (N <= 32 768): 64 envs per 256-thread block, their state in wave 0's
// registers for all K steps, as rollout_kernel<.., 64>.  Waves 1-3 do for the rollout what they do
// for one step in step_kernel_small: while wave 0 steps, they draw the step's randomness after
// sub-step 0 (reference-default shape with sensor noise, the HD_* layout) and compute every env's
// potential auto-reset speculatively (its draws are keyed by the env's RNG counter, which advances
// by one per env-step), leaving the parts that do not depend on the finished episode in LDS
// records: the reset pose, velocities, motor state, latency ring (RK_*), the domain randomisation,
// disturbance and level (RP_*), and the two reset sensor calls' held measurements and gyro normals
// (RO_*).  After one LDS barrier wave 0 only copies a record into a finishing env's registers and
// runs the two gyro updates that need the finished episode's body rates and gyro bias.  Per step:
// barrier A (wave 0 in sub-step 1 with HD, else at the top of the step; helpers write step k's
// records only after it, so wave 0 has read step k-1's) and barrier B (records and the finished
// envs' ballot in LDS).
enum { RK_P = 0, RK_Q = 3, RK_V = 7, RK_W = 10, RK_RPY = 13, RK_WB = 16, RK_X = 19, RK_ABUF = 23, RK_LA = 39,
       RK_WORDS = 43 };
enum { RP_DT = 0, RP_M = 1, RP_J = 2, RP_K0 = 5, RP_K1 = 6, RP_B = 7, RP_K = 11, RP_DSTB = 15, RP_LEVEL = 18,
       RP_LEVEL_IDX = 19, RP_WORDS = 20 };
enum { RO_HELD1 = 0, RO_NG1 = 10, RO_HELD2 = 19, RO_NG2 = 29, RO_WORDS = 38 };

// The fields of the kinematics and of the parameter record, one list each: op(word, field) for
// every field.  The helper waves store a record and the env wave loads it through the same list
// (small_roll_helper_step, small_roll_env_step).  Of the latency ring only the rows in use travel:
// the kinematics op also gets whether the field does (a reader zeroes the others).
template <class Op>
__device__ __forceinline__ void rk_fields(const KParams& P, Env& E, Op op) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        op(RK_P + c, E.p[c], true); op(RK_V + c, E.v[c], true); op(RK_W + c, E.w[c], true);
        op(RK_RPY + c, E.rpy[c], true); op(RK_WB + c, E.wb[c], true);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        op(RK_Q + c, E.q[c], true); op(RK_X + c, E.x[c], true); op(RK_LA + c, E.la[c], true);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) op(RK_ABUF + 4 * r + c, E.abuf[r][c], r < P.buf_size);
}
template <class Op>
__device__ __forceinline__ void rp_fields(Env& E, Op op) {
    op(RP_DT, E.dt); op(RP_M, E.m);
#pragma unroll
    for (int c = 0; c < 3; ++c) { op(RP_J + c, E.J[c]); op(RP_DSTB + c, E.dstb[c]); }
    op(RP_K0, E.k0); op(RP_K1, E.k1);
#pragma unroll
    for (int c = 0; c < 4; ++c) { op(RP_B + c, E.B[c]); op(RP_K + c, E.K[c]); }
    op(RP_LEVEL, E.level);
    float li = ib(E.level_idx);      // the level index travels as its bits
    op(RP_LEVEL_IDX, li);
    E.level_idx = bi(li);
}

// LDS records of one 64-env group of the small-N fused rollouts ([word][env] columns)
struct SmallRollLds {
    float* obs;          // [64][OD] the group's obs rows
    float* kin;          // [RK_WORDS][64]
    float* par;          // [RP_WORDS][64]
    float* ho;           // [RO_WORDS][64] (sensor noise only)
    float* draw;         // [HD_WORDS][64] (HD only)
    uint32_t* mask;      // [3] the group's finished envs (ballot of its env wave), the pose flag
};

// The env wave's part of one step of the small-N fused rollouts: the env-step (barrier A_k inside
// it with HD, else at the top), the ballot, barrier B_k, and a finishing env's reset copied from
// the helpers' records into its registers, its reset observation row into L.obs.
template <bool NOISE, bool DR, int PHYS, int SPEC>
__device__ __forceinline__ void small_roll_env_step(const KParams& P, const StepIO& io, uint32_t i, uint32_t lane,
                                                    bool live, Env& E, const SmallRollLds& L, const double* s_hjgrid) {
    constexpr int OL = NOISE ? 13 : 17;
    constexpr int OD = 2 * (OL + 4);
    constexpr bool HD = SPEC == 1 && NOISE;
    float* obs_row = L.obs + lane * OD;
    if (!HD) lds_barrier();                  // A_k (HD: inside the env-step, before sub-step 1)
    bool do_reset = false;
    ResetSeed rs;
    if (live)
        do_reset = step_env_body<NOISE, DR, PHYS, false, false, HD, 0, false, true>(P, io, i, E, obs_row, rs, s_hjgrid,
                                                                                    L.draw + lane);
    const uint64_t m = __ballot(do_reset);
    if (lane == 0) { L.mask[0] = (uint32_t)m; L.mask[1] = (uint32_t)(m >> 32); }
    lds_barrier();                           // B_k: the helpers' records of step k are in LDS
    if (do_reset) {
        const float stale[3] = {rs.wb[0], rs.wb[1], rs.wb[2]};   // the gyro LPF seed
        const float* kin = L.kin + lane;
        const float* par = L.par + lane;
        rk_fields(P, E, [&](int w, float& f, bool on) { f = on ? kin[w * 64] : 0.0f; });
#pragma unroll
        for (int c = 0; c < 4; ++c) E.xl[c] = 0.0f;
        E.ep_step = 0; E.aidx = 0; E.props_on = 0; E.la_view = 1;
        rp_fields(E, [&](int w, float& f) { f = par[w * 64]; });
        E.gust_left = 0;
        // the reset observation (reset_observe): two sensor calls, then the history row
        float o0[17], o1[17];
        if (NOISE) {
            const float* ho = L.ho + lane;
            float ng1[9], ng2[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) { ng1[c] = ho[(RO_NG1 + c) * 64]; ng2[c] = ho[(RO_NG2 + c) * 64]; }
#pragma unroll
            for (int c = 0; c < 3; ++c) E.lpf[c] = stale[c];
#pragma unroll
            for (int c = 0; c < 10; ++c) { o0[c] = ho[(RO_HELD1 + c) * 64]; o1[c] = ho[(RO_HELD2 + c) * 64]; }
#pragma unroll
            for (int c = 0; c < 10; ++c) E.held[c] = o1[c];
            gyro_update(P, E, ng1);
#pragma unroll
            for (int c = 0; c < 3; ++c) o0[10 + c] = E.lpf[c];
            gyro_update(P, E, ng2);
#pragma unroll
            for (int c = 0; c < 3; ++c) o1[10 + c] = E.lpf[c];
        } else {
            float o[17];
            plain_obs(E, o);
#pragma unroll
            for (int c = 0; c < 17; ++c) { o0[c] = o[c]; o1[c] = o[c]; }
        }
        float row[OD];
#pragma unroll
        for (int c = 0; c < OL; ++c) { row[c] = o0[c]; row[OL + 4 + c] = o1[c]; E.obs_prev[c] = o1[c]; }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            row[OL + c] = E.la[c]; row[2 * OL + 4 + c] = E.la[c];
            E.hact[0][c] = E.la[c]; E.hact[1][c] = E.la[c];
        }
        E.halias0 = E.halias1 = 1;
#pragma unroll
        for (int c = 0; c < OD; c += 2) *reinterpret_cast<float2*>(obs_row + c) = make_float2(row[c], row[c + 1]);
    }
}

// A helper wave's part of one step (wave 1-3 of a group): the HD draws of step k, barrier A_k, the
// speculative reset of every env of the group into the LDS records, barrier B_k, and the level a
// finishing env's new episode keeps.  ctr: the env's RNG counter at step k.
template <bool NOISE, bool DR, int PHYS, int SPEC>
__device__ __forceinline__ void small_roll_helper_step(const KParams& P, const Keys& Kh, uint32_t ctr, uint32_t gid,
                                                       uint32_t wave, uint32_t lane, bool live, float& lvl,
                                                       int& lvl_idx, const SmallRollLds& L) {
    constexpr bool HD = SPEC == 1 && NOISE;
    constexpr uint32_t PARAMS_WAVE = 3u;
    if (HD) {
        if (live) helper_step_draws(Kh, ctr, gid, wave, L.draw + lane);
    }
    if (NOISE && wave == 1 && lane == 0) L.mask[2] = 0u;     // the pose flag of step k
    lds_barrier();                               // A_k
    Env H;
    if (P.auto_reset && live) {
        const Rng gr{Kh, ctr, gid, TAG_RESET};
        auto params = [&]() {
            H.level = lvl;
            H.level_idx = lvl_idx;
            reset_params<DR, true>(P, H, gr);
            float* par = L.par + lane;
            rp_fields(H, [&](int w, float& f) { par[w * 64] = f; });
        };
        // the reset pose once, by wave 1, into the kinematics record; with sensor noise waves 2-3
        // read its position, velocity and attitude from there once wave 1 has set the flag (they
        // draw their sensor-call noise, and wave 3 the reset's parameters, meanwhile)
        if (wave == 1) {
            reset_kinematics<PHYS, true>(P, H, gr, gid);
            float* kin = L.kin + lane;
            rk_fields(P, H, [&](int w, float& f, bool on) { if (on) kin[w * 64] = f; });
            if (NOISE && lane == 0) lds_flag_set(L.mask + 2);
        } else if (NOISE) {
            HeldNoise hn;
            float ngs[9];
            held_noise(P, gr, wave == 2 ? 32u : 40u, hn, ngs);
            if (wave == PARAMS_WAVE) params();
            lds_flag_wait(L.mask + 2, P.tab);
            const float* kin = L.kin + lane;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                H.p[c] = kin[(RK_P + c) * 64]; H.v[c] = kin[(RK_V + c) * 64]; H.rpy[c] = kin[(RK_RPY + c) * 64];
            }
            float held[10];
            held_combine(H, hn, held);
            float* ho = L.ho + lane;
            const int hb = wave == 2 ? RO_HELD1 : RO_HELD2, nb = wave == 2 ? RO_NG1 : RO_NG2;
#pragma unroll
            for (int c = 0; c < 10; ++c) ho[(hb + c) * 64] = held[c];
#pragma unroll
            for (int c = 0; c < 9; ++c) ho[(nb + c) * 64] = ngs[c];
        }
        if (!NOISE && wave == PARAMS_WAVE) params();
    }
    lds_barrier();                               // B_k
    if (P.auto_reset && live && wave == PARAMS_WAVE) {
        const uint64_t mask = ((uint64_t)L.mask[1] << 32) | (uint64_t)L.mask[0];
        if ((mask >> lane) & 1ull) { lvl = H.level; lvl_idx = H.level_idx; }   // the new episode's level
    }
}

template <bool NOISE, bool DR, int PHYS, int SPEC>
__global__ void __launch_bounds__(256, 2) rollout_kernel_small(KParams P0, StepIO io0, uint32_t K, uint32_t act_stride) {
    const KParams P = shape_view<SPEC>(P0);
    constexpr int OL = NOISE ? 13 : 17;
    constexpr int OD = 2 * (OL + 4);
    constexpr bool HD = SPEC == 1 && NOISE;
    constexpr uint32_t PARAMS_WAVE = 3u;          // as small_roll_helper_step's
    __shared__ __align__(16) float s_obs[64 * OD];
    __shared__ float s_kin[RK_WORDS * 64];                 // [word][env]
    __shared__ float s_par[RP_WORDS * 64];
    __shared__ float s_ho[NOISE ? RO_WORDS * 64 : 1];
    __shared__ float s_draw[HD ? HD_WORDS * 64 : 1];
    __shared__ uint32_t s_mask[3];
    __shared__ double s_hjgrid[6 * HJ_PTS];
    const SmallRollLds L{s_obs, s_kin, s_par, s_ho, s_draw, s_mask};
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t base = blockIdx.x * 64u, i = base + lane, gid = P.gid_off + i;
    const bool live = i < P.N;
    const bool need_level = P.need_level || io0.level != nullptr;
    if (P.dstb_mode == DSTB_HJ_T) stage_hj_grid(P.tab->hj_grid, s_hjgrid);     // uniform branch
    const size_t n = P0.out_stride;              // rows per output slab (the whole population)
    if (wave == 0) {
        __builtin_amdgcn_s_setprio(3);
        Env E;
        if (live) load_env<NOISE, DR, PHYS>(P, io0.sf, i, E, need_level, /*with_hist=*/true);
        for (uint32_t k = 0; k < K; ++k) {
            const StepIO I0 = late_io(io0);
            const StepIO io = step_slab(I0, I0.act + (size_t)k * act_stride, k, n, OD);
            small_roll_env_step<NOISE, DR, PHYS, SPEC>(P, io, i, lane, live, E, L, s_hjgrid);
            // this wave's 64 rows, written by this wave only: its LDS writes land before its reads
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            write_obs_rows<64u, OD, 64u>(io0.obs + (size_t)k * n * OD + (size_t)base * OD, s_obs,
                                         P.N - base < 64u ? P.N - base : 64u, lane);
        }
        if (live) store_env<NOISE, DR, PHYS>(P, io0.sf, i, E, /*params_dirty=*/true);
        return;
    }
    // helper waves 1-3
    __builtin_amdgcn_s_setprio(0);
    uint32_t ctr = 0;
    float lvl = 0.0f;
    int lvl_idx = 0;
    if (live) helper_wave_init(P, Tile(io0.sf, P.N, i), wave == PARAMS_WAVE, need_level, ctr, lvl, lvl_idx);
    const Keys Kh = make_keys(P.key0, P.key1);
    for (uint32_t k = 0; k < K; ++k, ++ctr)
        small_roll_helper_step<NOISE, DR, PHYS, SPEC>(P, Kh, ctr, gid, wave, lane, live, lvl, lvl_idx, L);
}

// The collect loop in one launch at small N (N <= 32 768: the 8-GPU node shard, C2).  A 512-thread
// block holds two 64-env groups, each run as rollout_kernel_small runs its block (wave 0 of the
// group steps its envs with the state in registers, waves 1-3 compute the potential resets and the
// step's draws), and after each env-step all 8 waves run the policy forward, one 16-row tile each,
// on the block's 128 new observations (still in LDS), whose actions the next env-step reads.
// Per step: barriers A_k, B_k (rollout_kernel_small's), P_k (every reset row is in LDS) and Q_k
// (the step's actions are visible to the env waves).  LDS: the fragments (60.8 KB, staged once)
// and two groups' records (2 x 46.6 KB): one block per CU, 8 waves, as two blocks of
// step_kernel_small; 32 768 envs are one residency round of 256 blocks.  Outputs bit-identical
// to K cf2_collect_step launches (the same device code for both halves).
constexpr uint32_t CROLL_SMALL_BLOCK = 512;
template <bool NOISE, bool DR, int PHYS, int SPEC>
__global__ void __launch_bounds__(CROLL_SMALL_BLOCK, 1) collect_rollout_kernel_small(KParams P0, StepIO io0,
                                                                                    PolicyIO pio, uint32_t K) {
    static_assert(NOISE && SPEC == 1, "the fused collect kernels are built for the reference-default shape with noise");
    const KParams P = shape_view<SPEC>(P0);
    constexpr int OD = 34;
    constexpr uint32_t PARAMS_WAVE = 3u;          // as small_roll_helper_step's
    using PK = Packed<OD, CF2_POLICY_BF16X3>;
    static_assert(PK::TOTAL % 4 == 0, "float4 staging");
    __shared__ __align__(16) float s_frag[PK::TOTAL];
    __shared__ __align__(16) float s_obs[2][64 * OD];
    __shared__ float s_kin[2][RK_WORDS * 64];
    __shared__ float s_par[2][RP_WORDS * 64];
    __shared__ float s_ho[2][RO_WORDS * 64];
    __shared__ float s_draw[2][HD_WORDS * 64];
    __shared__ uint32_t s_mask[2][3];
    __shared__ double s_hjgrid[6 * HJ_PTS];
    const uint32_t tid = threadIdx.x, wv = tid >> 6, grp = wv >> 2, wave = wv & 3u, lane = tid & 63u;
    const uint32_t base = blockIdx.x * 128u, gbase = base + 64u * grp, i = gbase + lane, gid = P.gid_off + i;
    const bool live = i < P.N;
    const SmallRollLds L{s_obs[grp], s_kin[grp], s_par[grp], s_ho[grp], s_draw[grp], s_mask[grp]};
    if (P.dstb_mode == DSTB_HJ_T) stage_hj_grid(P.tab->hj_grid, s_hjgrid);     // uniform branch
    {
        const float4* src = reinterpret_cast<const float4*>(pio.w);
        float4* dst = reinterpret_cast<float4*>(s_frag);
        for (uint32_t q = tid; q < PK::TOTAL / 4; q += CROLL_SMALL_BLOCK) dst[q] = src[q];
    }
    __syncthreads();                             // the fragments are in LDS
    const size_t n = P0.out_stride;              // rows per output slab (the whole population)
    const uint32_t nrows = P.N - base < 128u ? P.N - base : 128u;    // rows of this block (> 0)
    // policy tile of this wave: block rows 16 wv .. 16 wv + 15 (group wv / 4, its rows 16 (wv & 3) ..)
    const uint32_t r16 = lane & 15u, trow = 16u * wv + r16;
    const int g = (int)(lane >> 4);
    const float* trow_lds = &s_obs[wv >> 2][(16u * (wv & 3u) + r16) * OD];
    auto policy_tile = [&](uint32_t k) {
        float ep[4];
        policy_noise(pio.key0, pio.key1, pio.counter + k, pio.row_offset + base + trow, ep);   // lanes 0-15 use it
        PolicyLane<OD, CF2_POLICY_BF16X3> CL;
        policy_lane_init<OD, CF2_POLICY_BF16X3>(s_frag + PK::O_BIAS, g, CL);
        ObsRegs<OD, CF2_POLICY_BF16X3, 1> Xc;
        obs_regs_from_lds(trow_lds, g, Xc);
        policy_standardize<OD, CF2_POLICY_BF16X3, 1>(s_frag + PK::O_BIAS, g, CL, Xc);
        f4v o[1];
        policy_layers<OD, CF2_POLICY_BF16X3, 0, 1>(s_frag, s_frag + PK::O_BIAS, s_frag + PK::O_L3, (int)lane, Xc, o);
        if (trow < nrows)
            policy_emit_eps<OD, CF2_POLICY_BF16X3, 0>(o[0], base + trow, g, CL, ep, 1,
                                                      pio.act + (size_t)(k + 1) * n * 4, pio.val + (size_t)(k + 1) * n,
                                                      pio.logp + (size_t)(k + 1) * n, nullptr);
    };
    // the block's rows of step k into its obs slab: this wave's 16 rows (read from LDS after P_k)
    auto write_rows = [&](uint32_t k) {
        const uint32_t r0 = 16u * wv;
        if (r0 >= nrows) return;
        const uint32_t nr = nrows - r0 < 16u ? nrows - r0 : 16u;
        const float2* src = reinterpret_cast<const float2*>(&s_obs[wv >> 2][16u * (wv & 3u) * OD]);
        float2* dst = reinterpret_cast<float2*>(io0.obs + (size_t)k * n * OD + (size_t)(base + r0) * OD);
        for (uint32_t q = lane; q < nr * (OD / 2); q += 64u) dst[q] = src[q];
    };
    if (wave == 0) {
        __builtin_amdgcn_s_setprio(3);
        Env E;
        if (live) load_env<NOISE, DR, PHYS>(P, io0.sf, i, E, P.need_level, /*with_hist=*/true);
        for (uint32_t k = 0; k < K; ++k) {
            const StepIO io = step_slab(late_io(io0), pio.act + (size_t)k * n * 4, k, n, OD);
            small_roll_env_step<NOISE, DR, PHYS, SPEC>(P, io, i, lane, live, E, L, s_hjgrid);
            lds_barrier();                       // P_k: every row of the block is in LDS
            write_rows(k);
            policy_tile(k);
            __syncthreads();                     // Q_k: step k + 1's actions are visible, s_obs is free
        }
        if (live) store_env<NOISE, DR, PHYS>(P, io0.sf, i, E, /*params_dirty=*/true);
        return;
    }
    // helper waves 1-3 of the group
    __builtin_amdgcn_s_setprio(0);
    uint32_t ctr = 0;
    float lvl = 0.0f;
    int lvl_idx = 0;
    if (live) helper_wave_init(P, Tile(io0.sf, P.N, i), wave == PARAMS_WAVE, P.need_level, ctr, lvl, lvl_idx);
    const Keys Kh = make_keys(P.key0, P.key1);
    for (uint32_t k = 0; k < K; ++k, ++ctr) {
        small_roll_helper_step<NOISE, DR, PHYS, SPEC>(P, Kh, ctr, gid, wave, lane, live, lvl, lvl_idx, L);
        lds_barrier();                           // P_k
        write_rows(k);
        policy_tile(k);
        __syncthreads();                         // Q_k
    }
}

template <bool NOISE, bool DR, int PHYS, int SPEC>
__global__ void __launch_bounds__(256) reset_kernel(KParams P0, float* __restrict__ sf,
                                                    const uint8_t* __restrict__ mask, float* __restrict__ obs) {
    const KParams P = shape_view<SPEC>(P0);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.N) return;
    if (mask && !mask[i]) return;
    reset_one<NOISE, DR, PHYS>(P, sf, i, obs);
}

// initial (pre-reset) state: AgentBase defaults, nominal params
__global__ void init_kernel(KParams P, float* __restrict__ sf) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.N) return;
    const Tile T(sf, P.N, i);
    const F4 z = f4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int g = 0; g < NG; ++g) T.st(g, z);
    T.st(0, f4(0.0f, 0.0f, 1.0f, 0.0f));                 // pos (0, 0, 1), quat x
    T.st(1, f4(0.0f, 0.0f, 1.0f, 0.0f));                 // quat (.., w = 1), vel x
    T.st(G_PARAM, f4(P.time_step, P.mass, P.ixx, P.iyy));
    T.st(G_PARAM + 1, f4(P.izz, P.ft0, P.ft1, P.B));
    T.st(G_PARAM + 2, f4(P.B, P.B, P.B, P.K));
    float level = P.level_fixed;
    int li = 0;
    if (P.level_mode == LEVEL_BOLTZMANN_T) {
        // construction-time Boltzmann() draw (hover_free.py:488), rng counter 0xFFFFFFFF
        const Keys K = make_keys(P.key0, P.key1);
        const Rng g{K, 0xFFFFFFFFu, P.gid_off + i, TAG_RESET};
        const U4 u = g.block(0);
        li = boltzmann_index(P, u01(u.x));
        level = P.tab->level_values[li];
    }
    T.st(G_LEVEL, f4(P.K, P.K, P.K, level));
    T.st(G_LEVEL_IDX, f4(ib(li), 0.0f, 0.0f, 0.0f));
}

// public snapshot field -> internal slot (cf2sim_internal.h)
// -1: motor A[j] (derived), -2: not stored in this configuration (the gyro LPF without noise)
__device__ __forceinline__ int pub_float_slot(int f, bool noise) {
    if (f < F_RPY) return f;                              // pos, quat, vel, omega: same slots
    if (f < F_MOTOR) return S_RPY + (f - F_RPY);
    if (f < F_LPF) return f;                              // motor, ou, abuf, bias: same slots
    if (f < F_HELD) return noise ? S_LPF + (f - F_LPF) : -2;
    if (f < F_OBS_PREV) return S_HELD + (f - F_HELD);
    if (f < F_HIST_ACT) return S_OBSP + (f - F_OBS_PREV);
    if (f < F_PARAM) return S_HACT + (f - F_HIST_ACT);
    if (f < F_DSTB) {                                     // dt m J k0 k1 | A[4] | B[4] K[4]
        const int k = f - F_PARAM;
        if (k < 7) return S_PARAM + k;
        if (k < 11) return -1;                            // A = 1 - B: derived, not stored
        return S_PARAM + k - 4;
    }
    if (f < F_LEVEL) return S_DSTB + (f - F_DSTB);
    if (f == F_LEVEL) return S_LEVEL;
    return S_MOTOR_LO + (f - F_MOTOR_LO);
}
__device__ __forceinline__ int pub_int_slot(int f) {
    switch (f) {
    case I_EP_STEP: return S_EP;
    case I_RNG: return S_RNG;
    case I_FLAGS: return S_FLAGS;
    case I_LEVEL: return S_LEVEL_IDX;
    default: return S_GUST;
    }
}
__device__ __forceinline__ size_t slot_index(uint32_t i, int slot) {     // in floats
    return (size_t)(i >> 6) * (NG * 256) + (size_t)(slot >> 2) * 256 + (i & 63u) * 4 + (slot & 3);
}
// The public snapshot is canonical: an env in the ring's compact form (FL_RING_COMPACT) exports
// ring rows 1 .. ring_rows - 1 and hact[1] from row 0, and its flag word without the bit; an import
// writes explicit rows and a clear bit.  ring_rows: the rows in use where the context's shape can
// go compact (ring_compact_shape), else 0.
__global__ void state_convert_kernel(uint32_t N, float* __restrict__ sf, float* __restrict__ pf,
                                     int32_t* __restrict__ pi, int to_public, int noise, int ring_rows) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const bool compact =
        to_public && ring_rows > 0 && (__float_as_int(sf[slot_index(i, S_FLAGS)]) & (int)FL_RING_COMPACT) != 0;
    for (int f = 0; f < NF; ++f) {
        int slot = pub_float_slot(f, noise != 0);
        if (compact && f >= F_ABUF + 4 && f < F_ABUF + 4 * ring_rows) slot = S_ABUF + ((f - F_ABUF) & 3);
        if (compact && f >= F_HIST_ACT + 4 && f < F_HIST_ACT + 8) slot = S_ABUF + (f - (F_HIST_ACT + 4));
        if (slot == -2) {    // not stored: exported as 0, ignored on import
            if (to_public) pf[(size_t)f * N + i] = 0.0f;
            continue;
        }
        if (slot < 0) {      // motor A[j]: exported as 1 - B[j], ignored on import
            if (to_public) pf[(size_t)f * N + i] = 1.0f - sf[slot_index(i, pub_float_slot(f + 4, noise != 0))];
            continue;
        }
        // With sensor noise o_{k-1} has 13 entries and S_LPF lies on the slots of entries 13..15: an
        // import takes the low-pass state from F_LPF alone, whatever the snapshot's unused entries hold.
        if (!to_public && noise != 0 && f >= F_OBS_PREV && slot >= S_LPF && slot < S_LPF + 3) continue;
        float* in = sf + slot_index(i, slot);
        if (to_public) pf[(size_t)f * N + i] = *in;
        else *in = pf[(size_t)f * N + i];
    }
    for (int f = 0; f < NI; ++f) {
        float* in = sf + slot_index(i, pub_int_slot(f));
        const int keep = f == I_FLAGS ? ~(int)FL_RING_COMPACT : ~0;
        if (to_public) pi[(size_t)f * N + i] = __float_as_int(*in) & keep;
        else *in = __int_as_float(pi[(size_t)f * N + i] & keep);
    }
}

// the grid nodes arrive by value in the kernarg segment (720 B): the stand-alone call needs no
// device table, allocation or host synchronisation
// one thread per grid node: the sign bits hj_signs would compute for any state nearest to it
__global__ void __launch_bounds__(256) hj_sign_table_kernel(const float* __restrict__ V, uint32_t total,
                                                            uint8_t* __restrict__ bits) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;
    const uint32_t t = k / (uint32_t)HJ_TABLE, c = k - t * (uint32_t)HJ_TABLE;
    int idx[6];
    uint32_t r = c;
#pragma unroll
    for (int d = 5; d >= 0; --d) { idx[d] = (int)(r % HJ_PTS); r /= HJ_PTS; }
    bits[k] = (uint8_t)hj_node_bits(V + (size_t)t * HJ_TABLE, (int)c, idx);
}

__global__ void hj_kernel(HjGrid G, double3 umax, const float* __restrict__ V, const float* __restrict__ states,
                          uint32_t n, float level, float* __restrict__ dstb, float* __restrict__ uopt) {
    __shared__ double s_grid[6 * HJ_PTS];
    stage_hj_grid(G.p, s_grid);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double st[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) st[d] = (double)states[(size_t)i * 6 + d];
    const unsigned bits = hj_signs(V, st, s_grid);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double um = k == 0 ? umax.x : (k == 1 ? umax.y : umax.z);
        const double dm = (double)level * um;
        dstb[(size_t)i * 3 + k] = (float)((bits >> k) & 1u ? -dm : dm);
        if (uopt) uopt[(size_t)i * 3 + k] = (float)((bits >> k) & 1u ? -um : um);
    }
}

// ------------------------------------------------------------------------------------
// host-side launch table
// ------------------------------------------------------------------------------------
// Blocks resident at once (CUs x blocks per CU at the kernel's VGPR / LDS use) of the large-N
// kernels of this configuration, queried once per context at cf2_create for the context's device
// (KParams::rb_*): the first block index past one residency round (step_kernel's issue priority)
// and the slice size of the fused rollout.
template <bool NOISE, bool DR, int PHYS, int SPEC>
static hipError_t occupancy_t(KParams& P) {
    int dev = 0, cus = 0, per_step = 0, per_roll = 0, per_collect = 0, per_croll_small = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_step, step_kernel<NOISE, DR, PHYS, SPEC>, STEP_BLOCK, 0);
    if (e == hipSuccess)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_roll, rollout_kernel<NOISE, DR, PHYS, SPEC>, STEP_BLOCK, 0);
    if constexpr (NOISE && SPEC == 1 && PHYS == PHYS_BULLET_T)
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_collect, collect_kernel<NOISE, DR, PHYS, SPEC>,
                                                             STEP_BLOCK, 0);
    if constexpr (NOISE && SPEC == 1 && PHYS == PHYS_BULLET_T)
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &per_croll_small, collect_rollout_kernel_small<NOISE, DR, PHYS, SPEC>, CROLL_SMALL_BLOCK, 0);
    if (e != hipSuccess) return e;
    P.rb_step = (uint32_t)(cus * (per_step > 0 ? per_step : 1));
    P.rb_roll = (uint32_t)(cus * (per_roll > 0 ? per_roll : 1));
    P.rb_collect = (uint32_t)(cus * (per_collect > 0 ? per_collect : 1));
    P.rb_croll_small = (uint32_t)(cus * (per_croll_small > 0 ? per_croll_small : 1));
    return hipSuccess;
}

// The store policies step_kernel is compiled for: the ones choose_store_policy can return
// (cf2sim_api.cpp; measured in profiles/store_policy_ab.txt).  cf2_create refuses any other
// (store_policy_compiled).  collect_kernel and rollout_kernel have one form, the plain policy's:
// with the parameter, write-through did not beat plain in every run (fused rollout 27.24-27.64 vs
// 26.82-27.53 us per env-step at 262 144 envs; collect 61.1-61.9 vs 62.3-64.3 us there, but
// 25.98-26.30 vs 25.88-26.30 us at 65 536), so their instances were removed again.
#define CF2_STORE_POLICIES(X)                                    \
    X(store_policy_pack(AUX_PLAIN, AUX_NT, AUX_PLAIN))           \
    X(store_policy_pack(AUX_NT, AUX_NT, AUX_PLAIN))              \
    X(store_policy_pack(AUX_WT, AUX_NT_WT, AUX_PLAIN))
bool store_policy_compiled(uint32_t packed) {
#define CF2_POL_IS(POL) if (packed == (POL)) return true;
    CF2_STORE_POLICIES(CF2_POL_IS)
#undef CF2_POL_IS
    return false;
}

// blocks of `block` threads (one env or item each) that cover n
static inline dim3 grid_of(uint32_t n, uint32_t block) { return dim3((n + block - 1) / block); }

template <bool NOISE, bool DR, int PHYS, int SPEC>
static hipError_t launch_step_t(const KParams& P, const StepIO& io, hipStream_t s, const PackIO& X = PackIO{}) {
    // small N (<= 32768 envs: at most one 64-env wave per two SIMDs with the helpers) runs 64 envs
    // per block, the other three waves computing the envs' potential resets meanwhile
    // (step_kernel_small); above that the helper waves would cost residency (65 536 envs: 15.5 ->
    // 24.7 us with 64-env blocks)
    if (P.N <= SMALL_N_MAX) {
        hipLaunchKernelGGL((step_kernel_small<NOISE, DR, PHYS, SPEC>), grid_of(P.N, 64), dim3(256), 0, s, P, io, X);
        return hipGetLastError();
    }
    const dim3 grid = grid_of(P.N, STEP_BLOCK), block(STEP_BLOCK);
    KParams Pl = P;
    Pl.late_block = P.rb_step;
    // the instance of the context's store policy (P.store_policy, cf2_create: e.g. nt state stores
    // once the env state plus the step's I/O no longer fit the 256 MB Infinity Cache between env-steps)
#define CF2_POL_LAUNCH(POL)                                                                              \
    if (P.store_policy == (POL)) {                                                                       \
        hipLaunchKernelGGL((step_kernel<NOISE, DR, PHYS, SPEC, (int)(POL)>), grid, block, 0, s, Pl, io, X); \
        return hipGetLastError();                                                                        \
    }
    CF2_STORE_POLICIES(CF2_POL_LAUNCH)
#undef CF2_POL_LAUNCH
    return hipErrorNotSupported;
}
template <bool NOISE, bool DR, int PHYS, int SPEC>
static hipError_t launch_collect_t(const KParams& P, const StepIO& io, const PolicyIO& pio, hipStream_t s) {
    if constexpr (!NOISE || SPEC != 1 || PHYS != PHYS_BULLET_T) {
        return hipErrorNotSupported;
    } else {
        if (P.N <= SMALL_N_MAX) {     // small N: 64-env blocks with helper waves (as launch_step_t)
            hipLaunchKernelGGL((collect_kernel_small<NOISE, DR, PHYS, SPEC>), grid_of(P.N, 64), dim3(256), 0, s, P,
                               io, pio);
            return hipGetLastError();
        }
        KParams Pl = P;
        Pl.late_block = P.rb_collect;
        hipLaunchKernelGGL((collect_kernel<NOISE, DR, PHYS, SPEC>), grid_of(P.N, STEP_BLOCK), dim3(STEP_BLOCK), 0, s, Pl,
                           io, pio);
        return hipGetLastError();
    }
}
// A slice's view of the population (envs e0 .. of a K-step launch, e0 a multiple of 64): the state
// view starts at the slice's first tile, the actions and each output at its first row, so the
// kernel sees its envs as 0..N-1.  od: floats per observation row.
static inline StepIO slice_view(const StepIO& io, uint32_t e0, uint32_t od) {
    StepIO s = io;
    s.sf = io.sf + (size_t)(e0 / 64u) * (NG * 256);
    if (io.act) s.act = io.act + (size_t)e0 * 4;
    s.obs = io.obs + (size_t)e0 * od;
    s.rew = io.rew + e0;
    s.done = io.done + e0;
    if (io.trunc) s.trunc = io.trunc + e0;
    if (io.cost) s.cost = io.cost + e0;
    if (io.level) s.level = io.level + e0;
    if (io.final_obs) s.final_obs = io.final_obs + (size_t)e0 * od;
    return s;
}
// The K-step launches process the envs in slices that fit one residency round (round_blocks blocks
// of epb envs resident at once): a slice's blocks run all K steps together, so no block waits K
// steps for a free slot.  Slices are balanced in size and run one after the other on the stream.
// launch(Ps, ios, e0, nb) launches the nb blocks of the slice that starts at env e0: Ps counts the
// slice's envs and continues the global ids, ios is its slice_view; every per-step output slab
// keeps the whole population's stride (Ps.out_stride).
template <class F>
static hipError_t for_each_slice(const KParams& P, const StepIO& io, uint32_t epb, uint32_t round_blocks, uint32_t od,
                                 F launch) {
    const uint32_t blocks = (P.N + epb - 1) / epb;
    if (round_blocks == 0) round_blocks = 1u;
    const uint32_t nslices = (blocks + round_blocks - 1) / round_blocks;
    const uint32_t per = (blocks + nslices - 1) / nslices;           // blocks per slice (balanced)
    for (uint32_t b0 = 0; b0 < blocks; b0 += per) {
        const uint32_t nb = blocks - b0 < per ? blocks - b0 : per;
        const uint32_t e0 = b0 * epb;
        KParams Ps = P;
        Ps.N = (P.N - e0 < nb * epb) ? P.N - e0 : nb * epb;
        Ps.gid_off = P.gid_off + e0;
        Ps.out_stride = P.N;
        launch(Ps, slice_view(io, e0, od), e0, nb);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
template <bool NOISE, bool DR, int PHYS, int SPEC>
static hipError_t launch_rollout_t(const KParams& P, const StepIO& io, uint32_t K, uint32_t act_stride, hipStream_t s) {
    // Small N: 64 envs per block, the other waves help with the resets (as launch_step_t).
    const uint32_t epb = P.N <= SMALL_N_MAX ? 64u : STEP_BLOCK;
    return for_each_slice(P, io, epb, P.rb_roll, NOISE ? 34u : 42u,
                          [&](const KParams& Ps, const StepIO& ios, uint32_t, uint32_t nb) {
        if (epb == 64u)
            hipLaunchKernelGGL((rollout_kernel_small<NOISE, DR, PHYS, SPEC>), dim3(nb), dim3(256), 0, s, Ps, ios, K,
                               act_stride);
        else
            hipLaunchKernelGGL((rollout_kernel<NOISE, DR, PHYS, SPEC>), dim3(nb), dim3(STEP_BLOCK), 0, s, Ps, ios, K,
                               act_stride);
    });
}
template <bool NOISE, bool DR, int PHYS, int SPEC>
static hipError_t launch_collect_rollout_t(const KParams& P, const StepIO& io, const PolicyIO& pio, uint32_t K,
                                           hipStream_t s) {
    if constexpr (!NOISE || SPEC != 1 || PHYS != PHYS_BULLET_T) {
        return hipErrorNotSupported;
    } else {
        constexpr uint32_t OD = 34;
        if (P.N > SMALL_N_MAX) {
            // large N: one collect_kernel launch per env-step.  A one-launch version (rollout_kernel's
            // env-step with the state in registers + this policy phase, 2 blocks per CU) was
            // bit-identical but slower at 262 144 envs, 65.0 against 60.3 us per env-step
            // (tools/variants/collect_rollout_large.hip.txt, profiles/r04_collect_ab.txt)
            for (uint32_t k = 0; k < K; ++k) {
                StepIO iok = step_slab(io, pio.act + (size_t)k * P.N * 4, k, P.N, OD);
                iok.obs = io.obs + (size_t)k * P.N * OD;
                PolicyIO pk = pio;
                pk.counter = pio.counter + k;
                pk.act = pio.act + (size_t)(k + 1) * P.N * 4;
                pk.val = pio.val + (size_t)(k + 1) * P.N;
                pk.logp = pio.logp + (size_t)(k + 1) * P.N;
                const hipError_t e = launch_collect_t<NOISE, DR, PHYS, SPEC>(P, iok, pk, s);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        }
        // small N: 128-env blocks of two helper-wave groups (collect_rollout_kernel_small), one per
        // CU, in slices of one residency round each (for_each_slice)
        return for_each_slice(P, io, 128u, P.rb_croll_small, OD,
                              [&](const KParams& Ps, const StepIO& ios, uint32_t e0, uint32_t nb) {
            PolicyIO ps = pio;
            ps.row_offset = pio.row_offset + e0;
            ps.act = pio.act + (size_t)e0 * 4;
            ps.val = pio.val + e0;
            ps.logp = pio.logp + e0;
            hipLaunchKernelGGL((collect_rollout_kernel_small<NOISE, DR, PHYS, SPEC>), dim3(nb), dim3(CROLL_SMALL_BLOCK), 0,
                               s, Ps, ios, ps, K);
        });
    }
}
template <bool NOISE, bool DR, int PHYS, int SPEC>
static hipError_t launch_reset_t(const KParams& P, float* sf, const uint8_t* mask, float* obs, hipStream_t s) {
    const dim3 grid = grid_of(P.N, 256), block(256);
    hipLaunchKernelGGL((reset_kernel<NOISE, DR, PHYS, SPEC>), grid, block, 0, s, P, sf, mask, obs);
    return hipGetLastError();
}

// SPEC 1 when the config has the reference-default Bullet env-step shape (see shape_view), SPEC 2
// for the same shape flown in multi-drone formations
static inline bool spec_default_shape(const KParams& P) {
    return P.phys == PHYS_BULLET_T && P.agg == 2 && P.obs_rate == 2 && P.buf_size == 2 && P.use_latency &&
           P.use_motor_dyn;
}

#define CF2_DISPATCH(FN, ...)                                                                          \
    do {                                                                                               \
        const int key = (P.noise ? 4 : 0) | (P.dr ? 2 : 0) | (P.phys == PHYS_SIMPLE_T ? 1 : 0);           \
        if (spec_default_shape(P) && P.num_drones == 1) {                                              \
            switch (key) {                                                                             \
            case 0: return FN<false, false, PHYS_BULLET_T, 1>(__VA_ARGS__);                            \
            case 2: return FN<false, true, PHYS_BULLET_T, 1>(__VA_ARGS__);                             \
            case 4: return FN<true, false, PHYS_BULLET_T, 1>(__VA_ARGS__);                             \
            default: return FN<true, true, PHYS_BULLET_T, 1>(__VA_ARGS__);                             \
            }                                                                                          \
        }                                                                                              \
        if (spec_default_shape(P)) {                                                                   \
            switch (key) {                                                                             \
            case 0: return FN<false, false, PHYS_BULLET_T, 2>(__VA_ARGS__);                            \
            case 2: return FN<false, true, PHYS_BULLET_T, 2>(__VA_ARGS__);                             \
            case 4: return FN<true, false, PHYS_BULLET_T, 2>(__VA_ARGS__);                             \
            default: return FN<true, true, PHYS_BULLET_T, 2>(__VA_ARGS__);                             \
            }                                                                                          \
        }                                                                                              \
        switch (key) {                                                                                 \
        case 0: return FN<false, false, PHYS_BULLET_T, 0>(__VA_ARGS__);                                \
        case 1: return FN<false, false, PHYS_SIMPLE_T, 0>(__VA_ARGS__);                                \
        case 2: return FN<false, true, PHYS_BULLET_T, 0>(__VA_ARGS__);                                 \
        case 3: return FN<false, true, PHYS_SIMPLE_T, 0>(__VA_ARGS__);                                 \
        case 4: return FN<true, false, PHYS_BULLET_T, 0>(__VA_ARGS__);                                 \
        case 5: return FN<true, false, PHYS_SIMPLE_T, 0>(__VA_ARGS__);                                 \
        case 6: return FN<true, true, PHYS_BULLET_T, 0>(__VA_ARGS__);                                  \
        default: return FN<true, true, PHYS_SIMPLE_T, 0>(__VA_ARGS__);                                 \
        }                                                                                              \
    } while (0)

#ifdef CF2_TIMING
extern "C" int cf2_debug_timing_buffer(uint64_t* dev) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_cf2_timing), &dev, sizeof(dev));
}
#endif
hipError_t query_occupancy(KParams& P) { CF2_DISPATCH(occupancy_t, P); }
hipError_t launch_step(const KParams& P, const StepIO& io, hipStream_t s) { CF2_DISPATCH(launch_step_t, P, io, s); }
hipError_t launch_step_packed(const KParams& P, const StepIO& io, const PackIO& pio, hipStream_t s) {
    CF2_DISPATCH(launch_step_t, P, io, s, pio);
}
hipError_t launch_rollout(const KParams& P, const StepIO& io, uint32_t K, uint32_t act_stride, hipStream_t s) {
    CF2_DISPATCH(launch_rollout_t, P, io, K, act_stride, s);
}
hipError_t launch_collect(const KParams& P, const StepIO& io, const PolicyIO& pio, hipStream_t s) {
    CF2_DISPATCH(launch_collect_t, P, io, pio, s);
}
hipError_t launch_collect_rollout(const KParams& P, const StepIO& io, const PolicyIO& pio, uint32_t K, hipStream_t s) {
    CF2_DISPATCH(launch_collect_rollout_t, P, io, pio, K, s);
}
hipError_t launch_reset(const KParams& P, float* sf, const uint8_t* mask, float* obs, hipStream_t s) {
    CF2_DISPATCH(launch_reset_t, P, sf, mask, obs, s);
}
// (physics_kernel has no SPEC instances: every SPEC of a configuration launches the same kernel)
template <bool NOISE, bool DR, int PHYS, int SPEC>
static hipError_t launch_physics_t(const KParams& P, float* sf, const float* act, const float* dstb, float dt_override,
                                   hipStream_t s) {
    const dim3 grid = grid_of(P.N, 256), block(256);
    hipLaunchKernelGGL((physics_kernel<NOISE, DR, PHYS>), grid, block, 0, s, P, sf, act, dstb, dt_override);
    return hipGetLastError();
}
hipError_t launch_physics(const KParams& P, float* sf, const float* act, const float* dstb, float dt_override,
                          hipStream_t s) {
    CF2_DISPATCH(launch_physics_t, P, sf, act, dstb, dt_override, s);
}
hipError_t launch_state_convert(const KParams& P, float* sf, float* state_f, int32_t* state_i, int to_public,
                                hipStream_t s) {
    const dim3 grid = grid_of(P.N, 256), block(256);
    const int ring_rows = P.use_latency != 0 && P.agg >= P.buf_size ? (int)P.buf_size : 0;
    hipLaunchKernelGGL(state_convert_kernel, grid, block, 0, s, P.N, sf, state_f, state_i, to_public, (int)P.noise,
                       ring_rows);
    return hipGetLastError();
}
hipError_t launch_init(const KParams& P, float* sf, hipStream_t s) {
    const dim3 grid = grid_of(P.N, 256), block(256);
    hipLaunchKernelGGL(init_kernel, grid, block, 0, s, P, sf);
    return hipGetLastError();
}
hipError_t launch_hj_sign_table(const float* V, uint32_t num_tables, uint8_t* bits, hipStream_t s) {
    const uint32_t total = num_tables * (uint32_t)HJ_TABLE;
    hipLaunchKernelGGL(hj_sign_table_kernel, grid_of(total, 256), dim3(256), 0, s, V, total, bits);
    return hipGetLastError();
}

hipError_t launch_hj(const HjGrid& G, const double umax[3], const float* V, const float* states, uint32_t n,
                     float level, float* dstb, float* uopt, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid = grid_of(n, 256), block(256);
    const double3 um = make_double3(umax[0], umax[1], umax[2]);
    hipLaunchKernelGGL(hj_kernel, grid, block, 0, s, G, um, V, states, n, level, dstb, uopt);
    return hipGetLastError();
}

}  // namespace cf2
