// cf2sim_reset.h -- episode reset: its three pieces, the auto-reset's seed, state stores and role split
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf2sim_internal.h"
#include "cf2sim_rng.h"
#include "cf2sim_draws.h"
#include "cf2sim_math.h"
#include "cf2sim_state.h"
#include "cf2sim_dynamics.h"
#include "cf2sim_sensing.h"
#include "cf2sim_kernarg.h"
#include "cf2sim_timing.h"

namespace cf2 {

// ------------------------------------------------------------------------------------
// reset (base.py:420-464 + task_specific_reset + apply_domain_randomization)
// ------------------------------------------------------------------------------------
// The reset in three pieces (reset_env runs them in order; the step kernel's auto-reset runs them
// on different waves, see block_epilogue):
//   reset_kinematics  initial pose / velocities (task_specific_reset hover_free.py:237-289), motor
//                     state and latency ring, last action, readback -- what the observation needs;
//   reset_params      domain randomisation (base.py:241-298), const-wind draw, Boltzmann level;
//   reset_observe     the two reset sensor calls (base.py:444-456 incl. the stale-rpy_dot LPF
//                     seed) and the history / observation row.
// where the reset-only parameters are read: TAB 1 = the device tables (P.tab; the fused rollout,
// whose register budget cannot hold them from kernel entry), 2 = the kernarg block re-read at the
// reset (late_reset: the large-N step kernel, where holding them from kernel entry spilled them
// to VGPR lanes), else the kernarg block as loaded at kernel entry
template <int TAB>
__device__ __forceinline__ decltype(auto) reset_src(const KParams& P) {
    if constexpr (TAB == 1) return (*P.tab);
    else if constexpr (TAB == 2) return late_reset(P);
    else return (P);
}

template <int PHYS, int TAB = 0, class G>
__device__ __forceinline__ void reset_kinematics(const KParams& P, Env& E, const G& g, uint32_t gid) {
    const U4 b0 = g.block(0), b1 = g.block(1), b2 = g.block(2), b3 = g.block(3);
    const uint32_t u[16] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w,
                            b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
    E.ep_step = 0;
    E.props_on = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) E.x[j] = E.xl[j] = 0.0f;
    E.aidx = 0;
    const auto& Tr = reset_src<TAB>(P);  // reset-only parameters
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) E.abuf[r][j] = 0.0f;
    float pos[3] = {Tr.init_xyz[0], Tr.init_xyz[1], Tr.init_xyz[2]};
    if (P.num_drones > 1) {
        float off[3];
        formation_offset(P, gid % (uint32_t)P.num_drones, off);
#pragma unroll
        for (int k = 0; k < 3; ++k) pos[k] += off[k];
    }
    float quat[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    float vel[3] = {0.0f, 0.0f, 0.0f}, rate[3] = {0.0f, 0.0f, 0.0f};
    if (P.reset_dist) {
#pragma unroll
        for (int k = 0; k < 3; ++k) pos[k] += -Tr.pos_lim + (Tr.pos_lim - -Tr.pos_lim) * u01(u[k]);
        float rpy[3];
        rpy[0] = -Tr.angle_lim + (Tr.angle_lim - -Tr.angle_lim) * u01(u[4]);
        rpy[1] = -Tr.angle_lim + (Tr.angle_lim - -Tr.angle_lim) * u01(u[5]);
        rpy[2] = -Tr.yaw_lim + (Tr.yaw_lim - -Tr.yaw_lim) * u01(u[3]);
        quat_from_euler(rpy, quat);
#pragma unroll
        for (int k = 0; k < 3; ++k) vel[k] = vel[k] + (-Tr.vel_lim + (Tr.vel_lim - -Tr.vel_lim) * u01(u[8 + k]));
        rate[0] = rate[0] + (-Tr.rate_lim + (Tr.rate_lim - -Tr.rate_lim) * u01(u[11]));
        rate[1] = rate[1] + (-Tr.rate_lim + (Tr.rate_lim - -Tr.rate_lim) * u01(u[12]));
        rate[2] = -Tr.yaw_rate_lim + (Tr.yaw_rate_lim - -Tr.yaw_rate_lim) * u01(u[7]);
        float nx[4];
        normals<4>(g, 4, nx);
#pragma unroll
        for (int j = 0; j < 4; ++j) E.x[j] = Tr.hover_x + Tr.motor_std * nx[j];
        float nb[16];
        normals<16>(g, 5, nb);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                E.abuf[r][j] = r < P.buf_size ? clampf(Tr.hover_action + Tr.action_std * nb[4 * r + j], -1.0f, 1.0f) : 0.0f;
    }
    abuf_last(P, E, E.la);
    E.la_view = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) { E.p[k] = pos[k]; E.v[k] = vel[k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) E.q[k] = quat[k];
    const M3 R0 = rotmat(quat);
    float ww[3];
    mtv(R0, rate, ww);
    if (PHYS == PHYS_BULLET_T) {
#pragma unroll
        for (int k = 0; k < 3; ++k) E.w[k] = ww[k];
        euler_from_quat(E.q, E.rpy);
        mtv(R0, E.w, E.wb);      // R(q) of the reset quaternion
    } else {
        euler_from_quat(E.q, E.rpy);
        mtv(R0, ww, E.wb);
#pragma unroll
        for (int k = 0; k < 3; ++k) E.w[k] = E.wb[k];
    }
}

template <bool DR, int TAB = 0, class G>
__device__ __forceinline__ void reset_params(const KParams& P, Env& E, const G& g) {
    E.dt = P.time_step; E.m = P.mass; E.J[0] = P.ixx; E.J[1] = P.iyy; E.J[2] = P.izz;
    E.k0 = P.ft0; E.k1 = P.ft1;
#pragma unroll
    for (int j = 0; j < 4; ++j) { E.B[j] = P.B; E.K[j] = P.K; }
    if (DR) {
        const auto& Tr = reset_src<TAB>(P);   // reset-only parameters
        const U4 d0 = g.block(9), d1 = g.block(10), d2 = g.block(11), d3 = g.block(12);
        const uint32_t d[16] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w,
                                d2.x, d2.y, d2.z, d2.w, d3.x, d3.y, d3.z, d3.w};
#define DRAW(b, ui) (Tr.dr_lo[b] + (Tr.dr_hi[b] - Tr.dr_lo[b]) * u01(d[ui]))
        E.dt = DRAW(0, 0); E.m = DRAW(1, 1);
        E.J[0] = DRAW(2, 2); E.J[1] = DRAW(3, 3); E.J[2] = DRAW(4, 4);
        E.k0 = DRAW(5, 5); E.k1 = DRAW(6, 6);
        if (P.use_motor_dyn) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float mtc = DRAW(7, 7 + j);
                const float t2w = DRAW(8, 11 + j);
                const float T = mtc < E.dt ? E.dt : mtc;
                E.B[j] = E.dt / T;             // A = 1 - B (apply_action's compensated form)
                E.K[j] = 0.028f * P.g_agent * t2w / 4.0f;
            }
        }
#undef DRAW
    }
    {
        const U4 w = g.block(13);
        if (P.dstb_mode == DSTB_CONST_T) {
            const uint32_t wu[3] = {w.x, w.y, w.z};
#pragma unroll
            for (int k = 0; k < 3; ++k) E.dstb[k] = (-1.0f + 2.0f * u01(wu[k])) * P.umax[k] * E.level;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) E.dstb[k] = 0.0f;
        }
        E.gust_left = 0;
    }
    if (P.level_mode == LEVEL_BOLTZMANN_T) {          // the new episode's level (after the const-wind draw)
        E.level_idx = boltzmann_index(P, u01(g.block(3).y));
        E.level = P.tab->level_values[E.level_idx];
    }
}

// stale: the finished episode's body rates (the gyro LPF seed); E.bias is the never-reset gyro bias.
// half: 0 = both calls and the whole observation row; 1 = the first call only, out[0 .. OL+4)
// (o_0 and A_0); 2 = the second call and out[OL+4 .. OD) (o_1, A_1), the first call's gyro walk
// only (its held measurement is not needed there).
template <bool NOISE, int HALF, class G>
__device__ __forceinline__ void reset_observe(const KParams& P, Env& E, const G& g, const float stale[3], float* out) {
    constexpr int OL = NOISE ? 13 : 17;
    if (NOISE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) E.lpf[k] = stale[k];
    }
    float o0[17], o1[17];
    compute_observation<NOISE>(P, E, g, 32, 0, o0, HALF != 2);
#pragma unroll
    for (int k = 0; k < OL; ++k) E.obs_prev[k] = o0[k];
    E.halias0 = E.halias1 = 1;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) E.hact[s][k] = E.la[k];
    if (HALF == 1) {
#pragma unroll
        for (int k = 0; k < OL; ++k) out[k] = o0[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) out[OL + k] = E.la[k];      // halias0: the action buffer's last entry
        return;
    }
    compute_observation<NOISE>(P, E, g, 40, 0, o1);
    if (HALF == 2) {
#pragma unroll
        for (int k = 0; k < OL; ++k) { out[OL + 4 + k] = o1[k]; E.obs_prev[k] = o1[k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) out[2 * OL + 4 + k] = E.la[k];
        E.halias0 = E.halias1;
#pragma unroll
        for (int k = 0; k < 4; ++k) E.hact[0][k] = E.hact[1][k];
        E.halias1 = E.la_view;
#pragma unroll
        for (int k = 0; k < 4; ++k) E.hact[1][k] = E.la[k];
        return;
    }
    compute_history<NOISE>(P, E, o1, out);
}

template <bool NOISE, bool DR, int PHYS, int TAB = 0, class G>
__device__ __forceinline__ void reset_env(const KParams& P, Env& E, const G& g, uint32_t gid, float* out) {
    const float stale[3] = {E.wb[0], E.wb[1], E.wb[2]};
    reset_kinematics<PHYS, TAB>(P, E, g, gid);
    const int level_idx0 = E.level_idx;
    const float level0 = E.level;
    reset_params<DR, TAB>(P, E, g);
    // reset_observe does not read the level; keep the redrawn one
    (void)level_idx0; (void)level0;
    reset_observe<NOISE, 0>(P, E, g, stale, out);
}

// What an auto-reset consumes from the finished episode (handed to the resetting lane in LDS, so
// the reset issues no global load behind the step's store burst)
struct ResetSeed {
    float wb[3], bias[3], ou[4], level;
    int level_idx;
    uint32_t ctr;
};
// as words of an LDS row (block_epilogue parks it in the finished env's own obs row, the counter
// in word SEED_CTR)
enum { SEED_WORDS = 13, SEED_CTR = 12 };

// The reset table of one chunk of nc <= C listed envs of a B-thread block, drawn by every thread
// of the block: a Philox block per (slot, env), Box-Muller applied to the halves the reset turns
// into normals (reset_slot_normal_*), stored at s_rand[slot][word][env], which is what
// TableRng{s_rand + e, C} reads.  env_of(e, ctr, te) gives listed env e's RNG counter and
// block-local index.  The caller puts a block barrier between the draws and the table's readers.
template <uint32_t B, uint32_t C, class F>
__device__ __forceinline__ void draw_reset_table(const KParams& P, uint32_t base, uint32_t tid, uint32_t nc,
                                                 uint32_t* s_rand, F env_of) {
    const Keys K = make_keys(P.key0, P.key1);
    for (uint32_t w = tid; w < nc * RESET_SLOTS; w += B) {
        const uint32_t sl = w / nc, e = w - sl * nc;
        uint32_t ctr, te;
        env_of(e, ctr, te);
        U4 u = philox(K, reset_block_of_slot((int)sl), ctr, P.gid_off + base + te, TAG_RESET);
        if (reset_slot_normal_xy((int)sl)) {
            float z0, z1;
            box_muller(u.x, u.y, z0, z1);
            u.x = __float_as_uint(z0); u.y = __float_as_uint(z1);
        }
        if (reset_slot_normal_zw((int)sl)) {
            float z2, z3;
            box_muller(u.z, u.w, z2, z3);
            u.z = __float_as_uint(z2); u.w = __float_as_uint(z3);
        }
        uint32_t* q = s_rand + sl * 4 * C + e;
        q[0] = u.x; q[C] = u.y; q[2 * C] = u.z; q[3 * C] = u.w;
    }
}

// Reset one env in place: reads only what a reset consumes from the finished episode (the
// stale body rates for the gyro LPF, the never-reset gyro bias and OU state, the RNG counter
// and the disturbance level), writes the reset observation row and the whole state.
template <bool NOISE, bool DR, int PHYS>
__device__ __forceinline__ void reset_one(const KParams& P, float* __restrict__ sf, uint32_t i, float* __restrict__ obs) {
    constexpr int OD = NOISE ? 34 : 42;
    const Tile T(sf, P.N, i);
    Env E;
    const F4 g0 = T.ld(0), g1 = T.ld(1), g2 = T.ld(2), g3 = T.ld(3), go = T.ld(G_OU);
    const float q[4] = {g0.w, g1.x, g1.y, g1.z}, w[3] = {g2.z, g2.w, g3.x};
    if (PHYS == PHYS_BULLET_T) {
        const M3 R = rotmat(q);
        mtv(R, w, E.wb);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) E.wb[k] = w[k];
    }
    if (NOISE) {
        const F4 b = T.ld(G_BIAS);
        E.bias[0] = b.x; E.bias[1] = b.y; E.bias[2] = b.z;
    }
    E.ou[0] = go.x; E.ou[1] = go.y; E.ou[2] = go.z; E.ou[3] = go.w;
    const uint32_t rng_ctr = (uint32_t)bi(g3.z);
    E.rng = rng_ctr;
    E.level = T.ld(G_LEVEL).w;
    E.level_idx = bi(T.ld(G_LEVEL_IDX).x);
    float o[OD];
    const Keys K = make_keys(P.key0, P.key1);
    const Rng g{K, rng_ctr, P.gid_off + i, TAG_RESET};
    reset_env<NOISE, DR, PHYS>(P, E, g, P.gid_off + i, o);
    E.rng = rng_ctr + 1;
    if (obs) write_obs<NOISE>(obs, i, o);
    store_env<NOISE, DR, PHYS>(P, sf, i, E, true);
}

// The state groups an auto-reset writes, in three sets (their union is store_env(params_dirty)):
//   kinematics: pose, velocities, counters (rng = ctr + 1), motor state, OU state (inherited from
//               the finished episode), latency ring, rpy (Simple)       -> groups 0-6(+ring), 12, 28
//   history:    gyro bias (+ gust_left 0), held measurement, action history, o_{k-1} + gyro LPF
//                                                                        -> groups 10, 14-19, 21-23
//   params:     domain randomisation, disturbance, level                -> groups 13, 24-27, 29
// (TT: the tile type, TileT<ST_AUX>: a kernel's reset stores carry the cache policy of its step stores,
// so no group of an env is left under two policies in one launch)
template <int PHYS, class TT>
__device__ __forceinline__ void store_reset_kinematics(const KParams& P, const TT& T, const Env& E, const float ou[4],
                                                       uint32_t ctr) {
    T.st(0, f4(E.p[0], E.p[1], E.p[2], E.q[0]));
    T.st(1, f4(E.q[1], E.q[2], E.q[3], E.v[0]));
    T.st(2, f4(E.v[1], E.v[2], E.w[0], E.w[1]));
    const int fl = (E.aidx & 15) | (1 << 4) | (1 << 5) | (E.la_view << 6) | (E.props_on << 7);   // halias0/1 = 1
    T.st(G_CORE3, f4(E.w[2], ib(0), ib((int)(ctr + 1u)), ib(fl)));
    T.st(G_MOTOR, f4(E.x[0], E.x[1], E.x[2], E.x[3]));
    if (P.use_motor_dyn) T.st(G_MOTOR_LO, f4(0.0f, 0.0f, 0.0f, 0.0f));
    T.st(G_OU, f4(ou[0], ou[1], ou[2], ou[3]));
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < P.buf_size) T.st(G_ABUF + r, f4(E.abuf[r][0], E.abuf[r][1], E.abuf[r][2], E.abuf[r][3]));
    if (PHYS == PHYS_SIMPLE_T) T.st(G_RPY, f4(E.rpy[0], E.rpy[1], E.rpy[2], 0.0f));
}
template <bool NOISE, class TT>
__device__ __forceinline__ void store_reset_history(const KParams& P, const TT& T, const Env& E) {
    if (NOISE || gust_mode(P))
        T.st(G_BIAS, f4(NOISE ? E.bias[0] : 0.0f, NOISE ? E.bias[1] : 0.0f, NOISE ? E.bias[2] : 0.0f, ib(0)));
    if (NOISE && P.held_persistent) {
        T.st(G_HELD, f4(E.held[0], E.held[1], E.held[2], E.held[3]));
        T.st(G_HELD + 1, f4(E.held[4], E.held[5], E.held[6], E.held[7]));
        T.st(G_HELD + 2, f4(E.held[8], E.held[9], 0.0f, 0.0f));
    }
    T.st(G_HACT, f4(E.hact[0][0], E.hact[0][1], E.hact[0][2], E.hact[0][3]));
    T.st(G_HACT + 1, f4(E.hact[1][0], E.hact[1][1], E.hact[1][2], E.hact[1][3]));
    store_obs_prev<NOISE>(T, E);
}
template <bool DR, class TT>
__device__ __forceinline__ void store_reset_params(const KParams& P, const TT& T, const Env& E) {
    if (dstb_stored(P)) T.st(G_DSTB, f4(E.dstb[0], E.dstb[1], E.dstb[2], 0.0f));
    if (DR) {
        T.st(G_PARAM, f4(E.dt, E.m, E.J[0], E.J[1]));
        T.st(G_PARAM + 1, f4(E.J[2], E.k0, E.k1, E.B[0]));
        T.st(G_PARAM + 2, f4(E.B[1], E.B[2], E.B[3], E.K[0]));
    }
    T.st(G_LEVEL, f4(E.K[1], E.K[2], E.K[3], E.level));
    T.st(G_LEVEL_IDX, f4(ib(E.level_idx), 0.0f, 0.0f, 0.0f));
}

// One quarter of an auto-reset (block_epilogue runs the four roles on four waves at once; the
// union of their stores is store_env(params_dirty) and of their row writes the reset
// observation, as reset_env + store_env produce them):
//   0: kinematics, motor state, ring           -> store_reset_kinematics
//   1: kinematics + the first sensor call      -> obs row o_0 | A_0
//   2: kinematics + the second sensor call     -> obs row o_1 | A_1; store_reset_history
//   3: domain randomisation, disturbance, level -> store_reset_params
// Roles 1 and 2 recompute the reset pose from the same table entries, so the critical path is one
// pose + one sensor call instead of the whole reset.
template <bool NOISE, bool DR, int PHYS, int TAB = 0, int ST_AUX = 0>
__device__ __forceinline__ void reset_role(const KParams& P, float* __restrict__ sf, uint32_t i, const ResetSeed& rs,
                                           const TableRng& g, float* __restrict__ obs_row, uint32_t role) {
    constexpr int OL = NOISE ? 13 : 17;
    const TileT<ST_AUX> T(sf, P.N, i);
    const uint32_t gid = P.gid_off + i;
    Env E;
    TSTAMP(6);   // role start (after the table-draw barrier)
#pragma unroll
    for (int k = 0; k < 3; ++k) { E.wb[k] = rs.wb[k]; E.bias[k] = rs.bias[k]; }
    const float stale[3] = {rs.wb[0], rs.wb[1], rs.wb[2]};
    if (role == 3) {
        E.level = rs.level;
        E.level_idx = rs.level_idx;
        reset_params<DR, TAB>(P, E, g);
        store_reset_params<DR>(P, T, E);
        return;
    }
    reset_kinematics<PHYS, TAB>(P, E, g, gid);
    TREADY("v"(E.q[3]), "v"(E.w[0]));
    TSTAMP(7);   // reset pose computed
    if (role == 0) {
        store_reset_kinematics<PHYS>(P, T, E, rs.ou, rs.ctr);
        return;
    }
    if (role == 1) {
        float o[OL + 4];
        reset_observe<NOISE, 1>(P, E, g, stale, o);
#pragma unroll
        for (int k = 0; k < OL + 4; ++k) obs_row[k] = o[k];
        return;
    }
    float o[2 * (OL + 4)];
    reset_observe<NOISE, 2>(P, E, g, stale, o);
#pragma unroll
    for (int k = OL + 4; k < 2 * (OL + 4); ++k) obs_row[k] = o[k];
    TREADY("v"(o[2 * (OL + 4) - 1]));
    TSTAMP(8);   // role 2: second sensor call + history done
    store_reset_history<NOISE>(P, T, E);
}

}  // namespace cf2
