// cf2sim_step.h -- the env-step on a loaded Env (step_env_body) and from the state in memory (step_env)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf2sim_internal.h"
#include "cf2sim_rng.h"
#include "cf2sim_draws.h"
#include "cf2sim_math.h"
#include "cf2sim_hj.h"
#include "cf2sim_state.h"
#include "cf2sim_dynamics.h"
#include "cf2sim_sensing.h"
#include "cf2sim_kernarg.h"
#include "cf2sim_timing.h"
#include "cf2sim_reset.h"

namespace cf2 {

// Compile-time view of the env-step shape.  SPEC 1 is the reference default for the Bullet envs
// (aggregate_phy_steps 2, obs_rate 2, buf_size 2, latency + motor dynamics on): the shape fields
// of a local KParams copy become constants, so the sub-step loop unrolls, the sensor-call parity
// and the latency-ring index resolve statically and the dead sub-step draws drop out.
template <int SPEC>
__device__ __forceinline__ KParams shape_view(const KParams& P) {
    KParams Q = P;
    if (SPEC == 1 || SPEC == 2) {
        Q.agg = 2; Q.obs_rate = 2; Q.buf_size = 2; Q.use_latency = 1; Q.use_motor_dyn = 1; Q.held_persistent = 0;
    }
    if (SPEC == 1) { Q.num_drones = 1; Q.downwash_on = 0; }   // single drones: formation code drops out
    return Q;
}

// One env-step of env i (aggregate_phy_steps physics sub-steps, observation, reward, done);
// returns whether the env finished and must be auto-reset.
// The env-step on a loaded Env.  STORE: write the state back (the one-step kernel: the physics
// state as soon as it is final, the rest at the end); the fused rollout keeps it in registers.
// HD (small-N kernel, reference-default shape with sensor noise): the draws after the first
// sub-step come from the helper waves' LDS table (hd = its column of this env, HD_* layout); the
// env wave joins the helpers' LDS barrier before its second sub-step.
template <bool NOISE, bool DR, int PHYS, bool STORE, bool SKIP_RESETTING = false, bool HD = false, int ST_AUX = 0,
          bool LATEP = false, bool LATEX = false>
// LATEP: the epilogue's, the final sensor call's parameters and the output pointers re-read where
// used (step_kernel, collect_kernel); LATEX: the epilogue's, the sensor call's and the physics
// sub-steps' parameters (the fused rollout, whose output pointers change per env-step)
__device__ __forceinline__ bool step_env_body(const KParams& P, const StepIO& io, uint32_t i, Env& E,
                                              float* __restrict__ obs_row, ResetSeed& rs, const double* hj_grid,
                                              const float* hd = nullptr) {
    constexpr int OL = NOISE ? 13 : 17;
    constexpr int OD = 2 * (OL + 4);
    const uint32_t gid = P.gid_off + i;
    const float4 a4 = reinterpret_cast<const float4*>(io.act)[i];
    TREADY("v"(E.p[0]), "v"(E.obs_prev[OL - 1]), "v"(E.hact[1][3]), "v"(E.K[3]), "v"(a4.w), "v"(E.rng));
    TSTAMP(1);   // every state load has landed
    const float a[4] = {a4.x, a4.y, a4.z, a4.w};
    const Keys K = make_keys(P.key0, P.key1);
    const Rng g{K, E.rng, gid, TAG_STEP};
    // reference-default shape: the final (full) sensor call's blocks are drawn up front (RowRng)
    const bool pre_final = !HD && NOISE && P.agg == 2 && P.obs_rate == 2;
    const uint32_t* hdw = reinterpret_cast<const uint32_t*>(hd);
    const uint32_t fbase = 8u + 8u * (uint32_t)P.agg;
    if (pre_final) {
        uint32_t* row = reinterpret_cast<uint32_t*>(obs_row);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const U4 u = g.block(fbase + b);
            float z0, z1, z2, z3;
            box_muller(u.x, u.y, z0, z1);
            box_muller(u.z, u.w, z2, z3);
            row[4 * b] = __float_as_uint(z0); row[4 * b + 1] = __float_as_uint(z1);
            row[4 * b + 2] = __float_as_uint(z2); row[4 * b + 3] = __float_as_uint(z3);
        }
        {
            const U4 u = g.block(fbase + 4);
            float z0, z1;
            box_muller(u.x, u.y, z0, z1);
            row[16] = __float_as_uint(z0); row[17] = __float_as_uint(z1); row[18] = u.z; row[19] = u.w;
        }
        {
            const U4 u = g.block(fbase + 5);
            row[20] = u.x; row[21] = u.y; row[22] = u.z; row[23] = u.w;
        }
    }
    if (PHYS == PHYS_BULLET_T) {
        euler_from_quat(E.q, E.rpy);
        const M3 R = rotmat(E.q);
        mtv(R, E.w, E.wb);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) E.wb[k] = E.w[k];
    }
    const float level_used = E.level;
    // disturbance (once per env-step, held for all sub-steps)
    float d[3] = {0.0f, 0.0f, 0.0f};
    switch (P.dstb_mode) {
    case DSTB_EXTERNAL_T:
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = io.dstb[(size_t)i * 3 + k];
        break;
    case DSTB_UNIFORM_T: {
        const U4 u = g.block(0);
        const uint32_t uu[3] = {u.x, u.y, u.z};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d[k] = (float)(-P.uni_hi[k] + (P.uni_hi[k] - -P.uni_hi[k]) * (double)u01(uu[k]));
        break;
    }
    case DSTB_CONST_T:
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = E.dstb[k];
        break;
    case DSTB_GUST_T: {
        const U4 u = g.block(0);
        const float was[3] = {E.dstb[0], E.dstb[1], E.dstb[2]};       // as loaded
        if (E.gust_left == 0 && u01(u.x) < P.gust_p) {
            E.gust_left = P.gust_dur;
            const float mag = P.gust_max * u01(u.y);
#pragma unroll
            for (int k = 0; k < 3; ++k) E.dstb[k] = ((u.z >> k) & 1u ? -1.0f : 1.0f) * mag * P.umax[k];
        }
        if (E.gust_left > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = E.dstb[k];
            E.gust_left -= 1;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) E.dstb[k] = 0.0f;
        }
        // compared bitwise here, so that one flag and not the loaded words stays live to store_core
        E.dstb_dirty = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) E.dstb_dirty |= __float_as_uint(E.dstb[k]) != __float_as_uint(was[k]);
        break;
    }
    case DSTB_HJ_T: {
        const int t = P.level_mode == LEVEL_FIXED_T ? P.tab->table_of_level[0] : P.tab->table_of_level[E.level_idx & 31];
        if (t >= 0 && P.V != nullptr) {
            float e[3];
            quat2euler(E.q, e);
            const double st[6] = {(double)e[0], (double)e[1], (double)e[2], (double)E.wb[0], (double)E.wb[1], (double)E.wb[2]};
            // the node's sign bits were derived from its 7 taps once per table (cf2_bind_hj_tables):
            // one byte gathered per env-step instead of 7 scattered floats of the 45.6 MB table
            int idx[6];
            const int c = hj_node(st, hj_grid, idx);
            const unsigned bits = P.hj_bits[(size_t)t * HJ_TABLE + (size_t)c];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float dm = (float)((double)E.level * (double)P.umax_d[k]);
                d[k] = (bits >> k) & 1u ? -dm : dm;
            }
        }
        break;
    }
    default: break;
    }
#pragma unroll 4
    for (int s = 0; s < P.agg; ++s) {
        float on[4];
        if (HD && s == 1) normals<4>(RowRng<64>{hdw + HD_OU1 * 64, 2}, 2, on);
        else normals<4>(g, 1 + s, on);
        float dw = 0.0f;
        if (PHYS == PHYS_BULLET_T && P.num_drones > 1 && P.downwash_on)
            dw = downwash(P, E.p, gid % (uint32_t)P.num_drones);   // mates' positions before this sub-step
        if (PHYS == PHYS_BULLET_T) bullet_substep(late_physics_if<LATEX>(P), E, a, d, on, E.ep_step == 0 && s == 0 && !E.props_on, dw);
        else simple_substep(late_physics_if<LATEX>(P), E, a, on);
        float dummy[17];
        // a sub-step's held measurement reaches an observation only if the final measurement
        // of the env-step is not a full one (aggregate_phy_steps % obs_rate != 0)
        if (HD && s == 0) {
            // compute_observation of this full call with its held part dead: the gyro update alone
            lds_barrier();                                   // the helper waves' draws are in LDS
            float ng[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) ng[k] = hd[(HD_GYRO0 + k) * 64];
            gyro_update(P, E, ng);
        } else if (HD && s == 1) {
            compute_observation<NOISE>(P, E, RowRng<64>{hdw + HD_GYRO1 * 64, 16}, 16, E.ep_step * P.agg + s, dummy, false);
        } else {
            compute_observation<NOISE>(P, E, g, 8 + 8 * s, E.ep_step * P.agg + s, dummy, P.held_persistent != 0);
        }
    }
    // the history (o_{k-1}, last actions) is only read by compute_history: the one-step kernel
    // loads it after the physics, so its 21 registers are not live across the sub-steps (the final
    // sensor call hides the load latency; -0.6 us at 262144 envs)
    if (STORE) load_hist<NOISE>(Tile(io.sf, P.N, i), E);
    float onx[17];
    TREADY("v"(E.q[3]), "v"(E.lpf[2]));
    TSTAMP(2);   // physics sub-steps done
    if (HD) {
        compute_observation<NOISE>(P, E, RowRng<64>{hdw + HD_FINAL * 64, fbase}, fbase, (E.ep_step + 1) * P.agg, onx);
    } else if (pre_final) {
        const RowRng<1> gr{reinterpret_cast<const uint32_t*>(obs_row), fbase};
        compute_observation<NOISE>(late_sensor_if<LATEP || LATEX>(P), E, gr, fbase, (E.ep_step + 1) * P.agg, onx);
    } else {
        compute_observation<NOISE>(late_sensor_if<LATEP || LATEX>(P), E, g, fbase, (E.ep_step + 1) * P.agg, onx);
    }
    // LATEP (the large-N step kernel): the epilogue's parameters re-read here (late_epilogue)
    const auto& PL = late_epilogue_if<LATEP || LATEX>(P);
    const bool term = compute_done(PL, E);
    E.ep_step += 1;
    const bool trunc = P.max_steps > 0 && E.ep_step >= P.max_steps && !term;
    const bool done = term || trunc;
    const bool do_reset = done && P.auto_reset;
    // the physics state is final now: store it early so its registers free up before the
    // epilogue.  SKIP_RESETTING (the small-N kernel, whose reset stores follow an LDS-only
    // barrier): an env that auto-resets is not stored, its reset writes every group stored here,
    // so no two waves store one group in one launch.  The large-N kernel stores it anyway: its
    // resets follow __syncthreads, whose workgroup-scope release/acquire orders these stores before
    // the reset waves' stores to the same groups (skipping them cost 0.6 us there)
    if (STORE && !(SKIP_RESETTING && do_reset)) store_core<NOISE, DR, PHYS, ST_AUX, true>(P, io.sf, i, E);
    const auto& IL = late_outputs_if<LATEP>(io);
    {
        const float r = compute_reward(PL, E, a, term);
        const float cost = IL.cost ? compute_cost(PL, E) : 0.0f;    // info['cost'] only when asked for
        IL.rew[i] = r;
        IL.done[i] = (uint8_t)done;
        if (IL.trunc) IL.trunc[i] = (uint8_t)trunc;
        if (IL.cost) IL.cost[i] = cost;
        if (IL.level) IL.level[i] = level_used;
    }
    {
        float o[OD];
        compute_history<NOISE>(P, E, onx, o);
        // the block's obs rows are staged in LDS and written out coalesced by the kernel; a
        // reset env's row is overwritten there by its reset observation
#pragma unroll
        for (int k = 0; k < OD; k += 2)
            *reinterpret_cast<float2*>(obs_row + k) = make_float2(o[k], o[k + 1]);
        if (do_reset && IL.final_obs) write_obs<NOISE>(IL.final_obs, i, o);
    }
    if (do_reset) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { rs.wb[k] = E.wb[k]; rs.bias[k] = NOISE ? E.bias[k] : 0.0f; }
#pragma unroll
        for (int k = 0; k < 4; ++k) rs.ou[k] = E.ou[k];
        rs.level = E.level;
        rs.level_idx = E.level_idx;
        rs.ctr = E.rng;
    }
    E.rng += 1;
    if (STORE && !(SKIP_RESETTING && do_reset)) store_tail<NOISE, ST_AUX, true>(P, io.sf, i, E);
    TSTAMP(3);   // epilogue issued
    return do_reset;
}

template <bool NOISE, bool DR, int PHYS, bool SKIP_RESETTING = false, bool HD = false, int ST_AUX = 0,
          bool LATEP = false>
__device__ __forceinline__ bool step_env(const KParams& P, const StepIO& io, uint32_t i, float* __restrict__ obs_row,
                                         ResetSeed& rs, const double* hj_grid, const float* hd = nullptr) {
    Env E;
    // every state load is issued before the first state store: on gfx9 vmcnt also counts stores,
    // so a load issued after the state stores would wait for the whole store burst to drain (the
    // history is loaded after the physics sub-steps, still ahead of store_core, in step_env_body)
    load_env<NOISE, DR, PHYS>(P, io.sf, i, E, P.need_level || io.level != nullptr, /*with_hist=*/false);
    return step_env_body<NOISE, DR, PHYS, true, SKIP_RESETTING, HD, ST_AUX, LATEP>(P, io, i, E, obs_row, rs, hj_grid, hd);
}

}  // namespace cf2
