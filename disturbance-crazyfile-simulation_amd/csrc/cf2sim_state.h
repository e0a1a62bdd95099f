// cf2sim_state.h -- per-env register state, its AoSoA loads and stores, obs-row write-out, LDS barrier and flags
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf2sim_internal.h"

namespace cf2 {

// Coalesced write-out of a block's LDS-staged obs rows (contiguous in global memory) as
// non-temporal stores. The caller reads each row once (policy input, rollout storage), and the nt
// stores keep the rows from displacing the env state in the Infinity Cache between env-steps.
// Same-box A/B at 262 144 envs (tools/ab_rollout_nt.sh): the env-step 39.5 -> 38.5 us with the
// state streaming from HBM and 36.3 -> 36.0 us with it cache-resident; the rollout caller, whose
// policy reads these rows next, unchanged (bf16x3) to 1 % faster (fp32). Non-temporal loads of
// the actions helped the streaming case and cost +2 us in the resident one, so they were not kept.
// The full-block path is unrolled: every LDS read of the thread's chunks is issued before the first
// global store, so the chunks pay one LDS round trip instead of one each (the rolled loop waited
// lgkmcnt(0) before every store: ~3.2k cycles of the small-N env wave for its 9 chunks, r05 timeline).
// OBS_AUX: the stores' cache policy (AUX_*).  AUX_NT is the form above.  AUX_NT_WT adds sc1
// (write-through: the rows leave the XCD's L2 while the kernel runs instead of at its end; DESIGN.md
// section 3, "Store cache policy"); such a store goes through a buffer descriptor over the block's
// rows, the only store whose builtin takes the policy bits (its range check covers exactly the rows
// written).  obs_chunk_store: chunk k (16 or 8 B) of the block's rows.
template <int OBS_AUX, class V>
__device__ __forceinline__ void obs_chunk_store(V* dst, __amdgpu_buffer_rsrc_t r, uint32_t k, V v) {
    if constexpr (OBS_AUX == (int)AUX_NT) {
        __builtin_nontemporal_store(v, dst + k);
    } else if constexpr (sizeof(V) == 16) {
        typedef unsigned int u4x __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4x, v), r, (int)(k * 16u), 0, OBS_AUX);
    } else {
        typedef unsigned int u2x __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2x, v), r, (int)(k * 8u), 0, OBS_AUX);
    }
}
template <uint32_t EPB, uint32_t OD, uint32_t NT, int OBS_AUX = (int)AUX_NT>
__device__ __forceinline__ void write_obs_rows(float* dst, const float* s_obs, uint32_t nvalid, uint32_t tid) {
    typedef float f4x __attribute__((ext_vector_type(4)));
    typedef float f2x __attribute__((ext_vector_type(2)));
    constexpr uint32_t epb = EPB, od = OD, nthreads = NT;
    const __amdgpu_buffer_rsrc_t r =      // (unused, and dropped by the compiler, under AUX_NT)
        __builtin_amdgcn_make_buffer_rsrc(dst, 0, (int)(nvalid * OD * 4u), 0x00020000);
    if ((EPB * OD) % 4 == 0 && nvalid == epb && ((uintptr_t)dst & 15u) == 0) {
        constexpr uint32_t NQ = EPB * OD / 4, IT = (NQ + NT - 1) / NT;
        const f4x* src4 = reinterpret_cast<const f4x*>(s_obs);
        f4x* dst4 = reinterpret_cast<f4x*>(dst);
        f4x v[IT];
#pragma unroll
        for (uint32_t it = 0; it < IT; ++it) {
            const uint32_t k = tid + it * NT;
            v[it] = src4[k < NQ ? k : NQ - 1u];
        }
#pragma unroll
        for (uint32_t it = 0; it < IT; ++it) {
            const uint32_t k = tid + it * NT;
            if (NQ % NT == 0 || k < NQ) obs_chunk_store<OBS_AUX>(dst4, r, k, v[it]);
        }
    } else {
        const f2x* src2 = reinterpret_cast<const f2x*>(s_obs);
        f2x* dst2 = reinterpret_cast<f2x*>(dst);
        for (uint32_t k = tid; k < nvalid * od / 2; k += nthreads) obs_chunk_store<OBS_AUX>(dst2, r, k, src2[k]);
    }
}

// Block barrier for LDS hand-offs: the calling wave's LDS operations complete first, then
// s_barrier.  (On gfx950 __syncthreads lowers to the same two instructions -- its workgroup-scope
// fence needs no vmcnt wait -- but this form is explicit about what the hand-off relies on, and it
// has no fence semantics the compiler could move memory operations around.)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// A one-way hand-over between waves of a block without a block barrier: the producer's lane 0
// sets an LDS flag after the wave's LDS writes; consumers poll it (bounded, so a flag never set
// cannot hang the grid: the wait then records CF2_DEVERR_HANDOVER in the context's device error
// word, which cf2_device_errors reports, and BatchedCrazyflieEnv.check_device_errors raises on).
__device__ __forceinline__ void lds_flag_set(uint32_t* f) {
    __hip_atomic_store(f, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_flag_wait(uint32_t* f, const KTables* tab) {
    for (uint32_t it = 0; it < (1u << 22); ++it) {
        if (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u) return;
        __builtin_amdgcn_s_sleep(1);
    }
    atomicOr(const_cast<uint32_t*>(&tab->dev_err), (uint32_t)CF2_DEVERR_HANDOVER);
}

// One wave's part of the small-N kernel's write-out of its 64 obs rows: the float4 chunks that touch
// a row whose bit in mask is set (dirty: the reset observations the helper waves staged in rrow) or
// those that do not (from obs, the env-step's observations).  A chunk straddling a reset and a
// non-reset row is a dirty chunk, merged from both.
template <uint32_t OD>
__device__ __forceinline__ void write_obs_rows_part(float* dst, const float* s_obs, const float* s_rrow, uint64_t mask,
                                                    uint32_t nvalid, uint32_t lane, bool dirty) {
    typedef float f4x __attribute__((ext_vector_type(4)));
    typedef float f2x __attribute__((ext_vector_type(2)));
    if (nvalid == 64u && (64u * OD) % 4 == 0 && ((uintptr_t)dst & 15u) == 0) {
        // unrolled: the chunks' LDS reads all issue before the first store (one LDS round trip)
        constexpr uint32_t NQ = 64u * OD / 4, IT = (NQ + 63u) / 64u;
        const f4x* a4 = reinterpret_cast<const f4x*>(s_obs);
        const f4x* b4 = reinterpret_cast<const f4x*>(s_rrow);
        f4x* dst4 = reinterpret_cast<f4x*>(dst);
        f4x v[IT];
        bool on[IT];
#pragma unroll
        for (uint32_t it = 0; it < IT; ++it) {
            const uint32_t k = lane + 64u * it, kc = k < NQ ? k : NQ - 1u;
            const uint32_t r0 = 4u * kc / OD, r1 = (4u * kc + 3u) / OD;
            const bool s0 = (mask >> r0) & 1ull, s1 = (mask >> r1) & 1ull;
            on[it] = k < NQ && (s0 || s1) == dirty;
            if (!dirty) {
                v[it] = a4[kc];                  // clean chunks: no row of theirs reset
            } else {
                // a dirty chunk straddling a reset and a non-reset row is merged from both
                const f4x x = a4[kc], y = b4[kc];
                const uint32_t cut = r1 * OD - 4u * kc;        // first component of row r1
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) v[it][j] = (j >= cut ? s1 : s0) ? y[j] : x[j];
            }
        }
#pragma unroll
        for (uint32_t it = 0; it < IT; ++it)
            if (on[it]) __builtin_nontemporal_store(v[it], dst4 + lane + 64u * it);
    } else {
        const f2x* a2 = reinterpret_cast<const f2x*>(s_obs);
        const f2x* b2 = reinterpret_cast<const f2x*>(s_rrow);
        f2x* dst2 = reinterpret_cast<f2x*>(dst);
        for (uint32_t k = lane; k < nvalid * OD / 2; k += 64u) {
            const bool sr = (mask >> ((2u * k) / OD)) & 1ull;      // OD is even: a pair never spans rows
            if (sr != dirty) continue;
            __builtin_nontemporal_store((sr ? b2 : a2)[k], dst2 + k);
        }
    }
}

// ------------------------------------------------------------------------------------
// per-env register state
// ------------------------------------------------------------------------------------
struct Env {
    float p[3], q[4], v[3], w[3];   // w: world angular velocity (bullet) / body rates (simple)
    float rpy[3], wb[3];            // derived readback (drone.rpy, drone.rpy_dot)
    float x[4], xl[4], ou[4], abuf[4][4];   // motor state x + xl (compensated pair)
    float bias[3], lpf[3], held[10];
    float obs_prev[17];
    float hact[2][4];
    float dt, m, J[3], k0, k1, B[4], K[4];
    float dstb[3], level;
    int ep_step, aidx, halias0, halias1, la_view, props_on, level_idx, gust_left;
    uint32_t rng;
    float la[4];                    // drone.last_action
    bool compact;                   // the state in memory is in the ring's compact form (FL_RING_COMPACT)
    bool dstb_dirty;                // gust mode: the env-step changed dstb (store_core's store on change)
};

// ------------------------------------------------------------------------------------
// State access: AoSoA float4 groups through a buffer descriptor (cf2sim_internal.h, "internal
// state layout").  One VGPR offset (tile base + lane * 16) serves every group; the group
// offset g * 1024 is a constant the backend splits into the instruction's immediate offset
// and a shared SGPR.  Every access is one coalesced dwordx4 per lane (1 KB per wave).
// ------------------------------------------------------------------------------------
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
struct F4 { float x, y, z, w; };
__device__ __forceinline__ F4 f4(float x, float y, float z, float w) { return F4{x, y, z, w}; }
__device__ __forceinline__ float ib(int v) { return __int_as_float(v); }       // int field -> slot bits
__device__ __forceinline__ int bi(float v) { return __float_as_int(v); }

// ST_AUX: cache-policy bits of the state stores (AUX_*, cf2sim_internal.h; the context's policy
// picks the kernel instance, DESIGN.md section 3 "Store cache policy").  AUX_NT: the step kernel's
// stores when the working set exceeds the Infinity Cache -- at 1 Mi envs 185 -> 144 us, while at
// 262 144 envs (cache-resident) nt stores cost +3 us, as nt loads do at both sizes (the loads
// always use the default policy).  AUX_WT (sc1, write-through) where the working set is
// cache-resident: the lines stay in the caches and the data goes out while the kernel runs, not in
// the write-back of every dirty L2 line at the kernel's end (profiles/store_policy_ab.txt).
template <int ST_AUX = 0>
struct TileT {
    __amdgpu_buffer_rsrc_t r;
    uint32_t voff;
    __device__ __forceinline__ TileT(const void* base, uint32_t N, uint32_t i)
        : r(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(uint32_t)state_bytes(N), 0x00020000)),
          voff((i >> 6) * (uint32_t)(NG * 1024) + (i & 63u) * 16u) {}
    __device__ __forceinline__ F4 ld(int g) const {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(voff + (uint32_t)g * 1024u), 0, 0);
        return F4{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
    }
    // group ga in lanes where `first`, else gb: one load through a per-lane offset
    __device__ __forceinline__ F4 ld_sel(bool first, int ga, int gb) const {
        const uint32_t off = voff + (first ? (uint32_t)ga : (uint32_t)gb) * 1024u;
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
        return F4{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
    }
    __device__ __forceinline__ void st(int g, F4 f) const {
        const u32x4 v = {__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w)};
        __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)(voff + (uint32_t)g * 1024u), 0, ST_AUX);
    }
};
using Tile = TileT<>;

// G_LPF: with sensor noise the gyro LPF state shares the last o_{k-1} group (13 of its 16 slots
// are o_{k-1}): that group is read with the state, the other three with the history
enum : int { G_CORE3 = 3, G_MOTOR = 4, G_OU = 5, G_ABUF = 6, G_BIAS = 10, G_LPF = 19, G_RPY = 12, G_DSTB = 13,
             G_HACT = 14, G_OBSP = 16, G_HELD = 21, G_PARAM = 24, G_LEVEL = 27, G_MOTOR_LO = 28,
             G_LEVEL_IDX = 29 };

// The latency ring's compact form.  Where every env-step writes the whole ring (latency on and at
// least as many sub-steps as rows), every row holds the step's action afterwards, and so does
// hact[1] (compute_history).  Such a step stores the 16 B once, in G_ABUF + 0, and sets
// FL_RING_COMPACT in the env's flag word: rows r >= 1 and G_HACT + 1 are then stale in memory and
// every reader takes them from row 0 (load_env, load_hist, physics_kernel, state_convert_kernel).
// The condition is launch-uniform; a shape that fails it never sets or honours the bit.  Resets,
// whole-state stores (store_env) and imports write every row and clear the bit.
enum : int { FL_RING_COMPACT = 1 << 8 };       // bits 0-7: I_FLAGS (cf2sim_internal.h)
__device__ __forceinline__ bool ring_compact_shape(const KParams& P) {
    return P.use_latency != 0 && P.agg >= P.buf_size;
}
__device__ __forceinline__ bool gust_mode(const KParams& P) { return P.dstb_mode == DSTB_GUST_T; }
__device__ __forceinline__ bool dstb_stored(const KParams& P) {
    return P.dstb_mode == DSTB_CONST_T || P.dstb_mode == DSTB_GUST_T;
}

template <bool NOISE>
__device__ __forceinline__ void load_hist(const Tile& T, Env& E) {
    constexpr int OL = NOISE ? 13 : 17;
    // compact lanes: hact[1] is ring row 0.  In the one-step kernels this load is issued after the
    // physics and before store_core overwrites G_ABUF + 0; the wave's own later store to the same
    // address relies on the in-order vector-memory pipeline, as the other history loads do
    const F4 h0 = T.ld(G_HACT), h1 = T.ld_sel(E.compact, G_ABUF, G_HACT + 1);
    E.hact[0][0] = h0.x; E.hact[0][1] = h0.y; E.hact[0][2] = h0.z; E.hact[0][3] = h0.w;
    E.hact[1][0] = h1.x; E.hact[1][1] = h1.y; E.hact[1][2] = h1.z; E.hact[1][3] = h1.w;
#pragma unroll
    for (int g = 0; g < (NOISE ? 3 : (OL + 3) / 4); ++g) {     // noise: o_{k-1}[12] came with the LPF
        const F4 o = T.ld(G_OBSP + g);
        const float v[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * g + k < OL) E.obs_prev[4 * g + k] = v[k];
    }
}

template <bool NOISE, bool DR, int PHYS>
__device__ __forceinline__ void load_env(const KParams& P, const float* __restrict__ sf, uint32_t i, Env& E,
                                         bool need_level = true, bool with_hist = true) {
    const Tile T(sf, P.N, i);
    const F4 g0 = T.ld(0), g1 = T.ld(1), g2 = T.ld(2), g3 = T.ld(3), gx = T.ld(G_MOTOR), go = T.ld(G_OU);
    E.p[0] = g0.x; E.p[1] = g0.y; E.p[2] = g0.z; E.q[0] = g0.w;
    E.q[1] = g1.x; E.q[2] = g1.y; E.q[3] = g1.z; E.v[0] = g1.w;
    E.v[1] = g2.x; E.v[2] = g2.y; E.w[0] = g2.z; E.w[1] = g2.w;
    E.w[2] = g3.x;
    E.ep_step = bi(g3.y);
    E.rng = (uint32_t)bi(g3.z);
    const int fl = bi(g3.w);
    E.aidx = fl & 15; E.halias0 = (fl >> 4) & 1; E.halias1 = (fl >> 5) & 1; E.la_view = (fl >> 6) & 1;
    E.props_on = (fl >> 7) & 1;
    E.compact = ring_compact_shape(P) && (fl & FL_RING_COMPACT) != 0;
    E.dstb_dirty = false;
    E.x[0] = gx.x; E.x[1] = gx.y; E.x[2] = gx.z; E.x[3] = gx.w;
    {
        F4 xl = f4(0.0f, 0.0f, 0.0f, 0.0f);
        if (P.use_motor_dyn) xl = T.ld(G_MOTOR_LO);
        E.xl[0] = xl.x; E.xl[1] = xl.y; E.xl[2] = xl.z; E.xl[3] = xl.w;
    }
    E.ou[0] = go.x; E.ou[1] = go.y; E.ou[2] = go.z; E.ou[3] = go.w;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        F4 a = f4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r < P.buf_size) a = T.ld(G_ABUF + r);
        if (r >= 1 && r < P.buf_size && E.compact) a = f4(E.abuf[0][0], E.abuf[0][1], E.abuf[0][2], E.abuf[0][3]);
        E.abuf[r][0] = a.x; E.abuf[r][1] = a.y; E.abuf[r][2] = a.z; E.abuf[r][3] = a.w;
    }
    E.gust_left = 0;
    if (NOISE || gust_mode(P)) {
        const F4 b = T.ld(G_BIAS);
        if (NOISE) { E.bias[0] = b.x; E.bias[1] = b.y; E.bias[2] = b.z; }
        if (gust_mode(P)) E.gust_left = bi(b.w);
    }
    if (NOISE) {
        const F4 l = T.ld(G_LPF);
        E.obs_prev[12] = l.x; E.lpf[0] = l.y; E.lpf[1] = l.z; E.lpf[2] = l.w;
#pragma unroll
        for (int k = 0; k < 10; ++k) E.held[k] = 0.0f;
        if (P.held_persistent) {
            const F4 h0 = T.ld(G_HELD), h1 = T.ld(G_HELD + 1), h2 = T.ld(G_HELD + 2);
            const float hv[12] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y, h2.z, h2.w};
#pragma unroll
            for (int k = 0; k < 10; ++k) E.held[k] = hv[k];
        }
    }
    if (PHYS == PHYS_SIMPLE_T) {
        const F4 r = T.ld(G_RPY);
        E.rpy[0] = r.x; E.rpy[1] = r.y; E.rpy[2] = r.z;
    }
    if (dstb_stored(P)) {
        const F4 d = T.ld(G_DSTB);
        E.dstb[0] = d.x; E.dstb[1] = d.y; E.dstb[2] = d.z;
    } else {
        E.dstb[0] = E.dstb[1] = E.dstb[2] = 0.0f;
    }
    if (with_hist) load_hist<NOISE>(T, E);
    F4 lv = f4(0.0f, 0.0f, 0.0f, P.level_fixed);
    if (DR) {
        const F4 p0 = T.ld(G_PARAM), p1 = T.ld(G_PARAM + 1), p2 = T.ld(G_PARAM + 2);
        lv = T.ld(G_LEVEL);
        E.dt = p0.x; E.m = p0.y; E.J[0] = p0.z; E.J[1] = p0.w;
        E.J[2] = p1.x; E.k0 = p1.y; E.k1 = p1.z; E.B[0] = p1.w;
        E.B[1] = p2.x; E.B[2] = p2.y; E.B[3] = p2.z; E.K[0] = p2.w;
        E.K[1] = lv.x; E.K[2] = lv.y; E.K[3] = lv.z;
    } else {
        E.dt = P.time_step; E.m = P.mass; E.J[0] = P.ixx; E.J[1] = P.iyy; E.J[2] = P.izz;
        E.k0 = P.ft0; E.k1 = P.ft1;
#pragma unroll
        for (int k = 0; k < 4; ++k) { E.B[k] = P.B; E.K[k] = P.K; }
        if (need_level) lv = T.ld(G_LEVEL);
    }
    E.level = need_level ? lv.w : P.level_fixed;
    // the level index only matters where levels are redrawn (Boltzmann: the HJ table and the
    // reset keep it); a fixed-level env's index is 0 and its group is not read
    E.level_idx = need_level && P.level_mode != LEVEL_FIXED_T ? bi(T.ld(G_LEVEL_IDX).x) : 0;
}

// What a helper wave of the small-N kernels reads of its env's state at start-up: the RNG counter
// that keys the env's step and reset draws, and (the wave that draws the reset's parameters) the
// level and level index a reset keeps or redraws, as load_env reads them.  small_body reads the
// counter at entry and the level only after its draw barrier; the rollouts read both at entry.
__device__ __forceinline__ uint32_t helper_counter(const Tile& T) { return (uint32_t)bi(T.ld(G_CORE3).z); }
__device__ __forceinline__ void helper_level(const KParams& P, const Tile& T, bool need_level, float& level,
                                             int& level_idx) {
    level = need_level ? T.ld(G_LEVEL).w : P.level_fixed;
    level_idx = need_level && P.level_mode != LEVEL_FIXED_T ? bi(T.ld(G_LEVEL_IDX).x) : 0;
}
__device__ __forceinline__ void helper_wave_init(const KParams& P, const Tile& T, bool params_wave, bool need_level,
                                                 uint32_t& ctr, float& level, int& level_idx) {
    ctr = helper_counter(T);
    if (params_wave) helper_level(P, T, need_level, level, level_idx);
}

// state the physics sub-steps update (stored as soon as the last sub-step is done; group 3,
// which carries the counters, is stored with the history at the end of the step)
// STEP: the stores of an env-step (step_env_body): the ring in its compact form where the shape
// allows it (store_tail sets the bit), and in gust mode G_DSTB only in lanes whose torque changed
// (an onset, or the step after an expiry: ~2 % of env-steps at the default gust settings); the
// bytes in memory are the same either way.  Without STEP every group and every row is written.
template <bool NOISE, bool DR, int PHYS, int ST_AUX = 0, bool STEP = false>
__device__ __forceinline__ void store_core(const KParams& P, float* __restrict__ sf, uint32_t i, const Env& E) {
    const TileT<ST_AUX> T(sf, P.N, i);
    const bool once = STEP && ring_compact_shape(P);
    T.st(0, f4(E.p[0], E.p[1], E.p[2], E.q[0]));
    T.st(1, f4(E.q[1], E.q[2], E.q[3], E.v[0]));
    T.st(2, f4(E.v[1], E.v[2], E.w[0], E.w[1]));
    T.st(G_MOTOR, f4(E.x[0], E.x[1], E.x[2], E.x[3]));
    if (P.use_motor_dyn) T.st(G_MOTOR_LO, f4(E.xl[0], E.xl[1], E.xl[2], E.xl[3]));
    T.st(G_OU, f4(E.ou[0], E.ou[1], E.ou[2], E.ou[3]));
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < P.buf_size && !(once && r >= 1))
            T.st(G_ABUF + r, f4(E.abuf[r][0], E.abuf[r][1], E.abuf[r][2], E.abuf[r][3]));
    if (NOISE || gust_mode(P))
        T.st(G_BIAS, f4(NOISE ? E.bias[0] : 0.0f, NOISE ? E.bias[1] : 0.0f, NOISE ? E.bias[2] : 0.0f, ib(E.gust_left)));
    if (NOISE && P.held_persistent) {      // (the LPF state is stored with the history, store_tail)
        T.st(G_HELD, f4(E.held[0], E.held[1], E.held[2], E.held[3]));
        T.st(G_HELD + 1, f4(E.held[4], E.held[5], E.held[6], E.held[7]));
        T.st(G_HELD + 2, f4(E.held[8], E.held[9], 0.0f, 0.0f));
    }
    if (PHYS == PHYS_SIMPLE_T) T.st(G_RPY, f4(E.rpy[0], E.rpy[1], E.rpy[2], 0.0f));
    if (gust_mode(P) && (!STEP || E.dstb_dirty)) T.st(G_DSTB, f4(E.dstb[0], E.dstb[1], E.dstb[2], 0.0f));
}

// the o_{k-1} groups; with sensor noise the last one carries the gyro LPF state
template <bool NOISE, class TT>
__device__ __forceinline__ void store_obs_prev(const TT& T, const Env& E) {
    constexpr int OL = NOISE ? 13 : 17;
#pragma unroll
    for (int g = 0; g < (OL + 3) / 4; ++g) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = 4 * g + k < OL ? E.obs_prev[4 * g + k] : 0.0f;
        if (NOISE && G_OBSP + g == G_LPF) { v[1] = E.lpf[0]; v[2] = E.lpf[1]; v[3] = E.lpf[2]; }
        T.st(G_OBSP + g, f4(v[0], v[1], v[2], v[3]));
    }
}

// end of the step: history, counters (group 3 with the last angular-rate component)
// (STEP: as store_core; G_HACT + 0 is the previous hact[1] and is stored either way)
template <bool NOISE, int ST_AUX = 0, bool STEP = false>
__device__ __forceinline__ void store_tail(const KParams& P, float* __restrict__ sf, uint32_t i, const Env& E) {
    const TileT<ST_AUX> T(sf, P.N, i);
    const bool once = STEP && ring_compact_shape(P);
    T.st(G_HACT, f4(E.hact[0][0], E.hact[0][1], E.hact[0][2], E.hact[0][3]));
    if (!once) T.st(G_HACT + 1, f4(E.hact[1][0], E.hact[1][1], E.hact[1][2], E.hact[1][3]));
    store_obs_prev<NOISE>(T, E);
    const int fl = (E.aidx & 15) | (E.halias0 << 4) | (E.halias1 << 5) | (E.la_view << 6) | (E.props_on << 7) |
                   (once ? (int)FL_RING_COMPACT : 0);
    T.st(G_CORE3, f4(E.w[2], ib(E.ep_step), ib((int)E.rng), ib(fl)));
}

// whole state (reset paths): core + history + per-episode parameters + counters
template <bool NOISE, bool DR, int PHYS>
__device__ __forceinline__ void store_env(const KParams& P, float* __restrict__ sf, uint32_t i, const Env& E,
                                          bool params_dirty) {
    const Tile T(sf, P.N, i);
    store_core<NOISE, DR, PHYS>(P, sf, i, E);
    store_tail<NOISE>(P, sf, i, E);
    if (P.dstb_mode == DSTB_CONST_T && params_dirty) T.st(G_DSTB, f4(E.dstb[0], E.dstb[1], E.dstb[2], 0.0f));
    if (params_dirty) {
        if (DR) {
            T.st(G_PARAM, f4(E.dt, E.m, E.J[0], E.J[1]));
            T.st(G_PARAM + 1, f4(E.J[2], E.k0, E.k1, E.B[0]));
            T.st(G_PARAM + 2, f4(E.B[1], E.B[2], E.B[3], E.K[0]));
        }
        T.st(G_LEVEL, f4(E.K[1], E.K[2], E.K[3], E.level));
        T.st(G_LEVEL_IDX, f4(ib(E.level_idx), 0.0f, 0.0f, 0.0f));
    }
}

template <bool NOISE>
__device__ __forceinline__ void write_obs(float* __restrict__ dst, uint32_t i, const float* o) {
    constexpr int OD = NOISE ? 34 : 42;
    float2* d2 = reinterpret_cast<float2*>(dst + (size_t)i * OD);
#pragma unroll
    for (int k = 0; k < OD / 2; ++k) d2[k] = make_float2(o[2 * k], o[2 * k + 1]);
}

}  // namespace cf2
