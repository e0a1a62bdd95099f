// cf2sim_sensing.h -- sensor model, observation and history, done / reward / cost, Boltzmann level index
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf2sim_internal.h"
#include "cf2sim_rng.h"
#include "cf2sim_draws.h"
#include "cf2sim_math.h"
#include "cf2sim_state.h"

namespace cf2 {

// ------------------------------------------------------------------------------------
// observation / history / reward
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void omega_noise(const KParams& P, Env& E, const float* n, float om[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) E.bias[k] = P.pgd * E.bias[k] + P.sbgd * n[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) om[k] = E.wb[k] + E.bias[k] + P.gyro_rw * n[3 + k] + P.gyro_ton * n[6 + k];
}

// A full measurement's held part (noisy position, attitude quaternion and velocity,
// sensors.py:75-118) and its 9 gyro normals n[6..15) (bias walk, white noise, turn-on noise): what
// the measurement draws from stream blocks base..base+5.  The gyro part is applied by
// gyro_update, which needs the body rates, bias and LPF state of the moment.  Split in two so the
// draws can run before the state they perturb is known (the small-N kernel's helper waves):
// held_noise turns the draws into the position / velocity / rpy perturbations, held_combine adds
// them.  The velocity perturbation is rounded on its own (no fma into the sum), as the fp32
// restatement computes v + vel_std * n.
struct HeldNoise { float pn[3], vn[3], th[3]; };
template <class G>
__device__ __forceinline__ void held_noise(const KParams& P, const G& g, uint32_t base, HeldNoise& h, float ng[9]) {
    float n[18];
    normals<18>(g, base, n);
    const U4 ua = g.block(base + 4), ub = g.block(base + 5);
    const uint32_t up[3] = {ua.z, ua.w, ub.x}, ur[3] = {ub.y, ub.z, ub.w};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float uo = -P.pos_unif + (P.pos_unif - -P.pos_unif) * u01(up[k]);
        h.pn[k] = P.pos_std * n[k] + uo;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) h.vn[k] = opaque(P.vel_std * n[3 + k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float uo = -P.rot_unif + (P.rot_unif - -P.rot_unif) * u01(ur[k]);
        h.th[k] = P.rot_std * n[15 + k] + uo;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) ng[k] = n[6 + k];
}
__device__ __forceinline__ void held_combine(const Env& E, const HeldNoise& h, float held[10]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) held[k] = E.p[k] + h.pn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) held[7 + k] = E.v[k] + h.vn[k] + 0.0f;
    const float lo[3] = {-3.141592653589793f, -1.5707963267948966f, -3.141592653589793f};
    float rot[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) rot[k] = clampf(E.rpy[k] + h.th[k], lo[k], -lo[k]);
    quat_from_euler_obs(rot, held + 3);
}
template <class G>
__device__ __forceinline__ void held_measurement(const KParams& P, const Env& E, const G& g, uint32_t base,
                                                 float held[10], float ng[9]) {
    HeldNoise h;
    held_noise(P, g, base, h, ng);
    held_combine(E, h, held);
}

// gyro of one sensor call: bias walk + noise on the body rates, then the gyro low-pass filter
// (sensors.py:121-134, utils.py:102-105); ng = the call's 9 gyro normals
__device__ __forceinline__ void gyro_update(const KParams& P, Env& E, const float ng[9]) {
    float om[3];
    omega_noise(P, E, ng, om);
#pragma unroll
    for (int k = 0; k < 3; ++k) E.lpf[k] = (1.0f - P.lpf_ratio) * E.lpf[k] + P.lpf_gain * P.lpf_ratio * om[k];
}

// the noise-free observation, 17 wide: position, attitude quaternion, velocity, body rates, last action
__device__ __forceinline__ void plain_obs(const Env& E, float* o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = E.p[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[3 + k] = E.q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[7 + k] = E.v[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[10 + k] = E.wb[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[13 + k] = E.la[k];
}

// need_held = false: the held measurement of this call is dead (it is overwritten by a later
// full measurement before any observation is emitted), so a full measurement only advances the
// gyro (bias walk + LPF) and draws just the gyro normals n[6..15) of its stream positions.
template <bool NOISE, class G>
__device__ __forceinline__ void compute_observation(const KParams& P, Env& E, const G& g, uint32_t base,
                                                    int iteration, float* obs, bool need_held = true) {
    if (!NOISE) {
        plain_obs(E, obs);
        return;
    }
    const bool full = (uint32_t)iteration % (uint32_t)P.obs_rate == 0u;
    if (full && !need_held) {
        float n[18];
        normals_range<6, 15>(g, base, n);
        gyro_update(P, E, n + 6);
    } else if (full) {
        float held[10], ng[9];
        held_measurement(P, E, g, base, held, ng);
        gyro_update(P, E, ng);
#pragma unroll
        for (int k = 0; k < 10; ++k) E.held[k] = held[k];
    } else {
        float n[9];
        normals<9>(g, base, n);
        gyro_update(P, E, n);
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) obs[k] = E.held[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) obs[10 + k] = E.lpf[k];
}

__device__ __forceinline__ bool compute_done(const KParams& P, const Env& E) {
    const bool rp = fabsf(E.rpy[0]) > P.done_rp || fabsf(E.rpy[1]) > P.done_rp;
    bool rt = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) rt |= (180.0f * fabsf(E.wb[k]) * (1.0f / 3.141592653589793f)) > P.done_rate_deg;   // DIV_NOTE
    return rp || rt || (E.p[2] < P.done_zmin);
}

__device__ __forceinline__ float compute_reward(const KParams& P, const Env& E, const float a[4], bool done) {
    float na[4], ad[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { na[k] = 0.5f * (clampf(a[k], -1.0f, 1.0f) + 1.0f); ad[k] = a[k] - E.la[k]; }
    const float nna = sqrt_fast(na[0] * na[0] + na[1] * na[1] + na[2] * na[2] + na[3] * na[3]);
    const float nad = sqrt_fast(ad[0] * ad[0] + ad[1] * ad[1] + ad[2] * ad[2] + ad[3] * ad[3]);
    float dr[3], dw[3], dp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        dr[k] = E.rpy[k] - P.target_rpy[k];
        dw[k] = E.wb[k] - P.target_rate[k];
        dp[k] = E.p[k] - P.target_pos[k];
    }
    float pen = 0.0f;
    pen += P.pen_angle * norm3(dr);
    pen += P.pen_arp * nad;
    pen += P.pen_spin * norm3(dw);
    pen += P.pen_vel * norm3(E.v);
    pen += P.pen_action * nna;
    pen += done ? P.pen_term : 0.0f;
    const float zd = P.pen_z * fabsf(E.p[2] - P.target_pos[2]);
    const float dist = P.pen_dist * norm3(dp);
    return -pen - zd - dist;
}

__device__ __forceinline__ float compute_cost(const KParams& P, const Env& E) {
    float c = 0.0f;
    if (fabsf(E.p[0]) > P.cost_xy || fabsf(E.p[1]) > P.cost_xy || E.p[2] > P.cost_z) c = 1.0f;
    if (fabsf(E.rpy[0]) > P.cost_rp || fabsf(E.rpy[1]) > P.cost_rp) c = 1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) if (fabsf(E.wb[k]) > P.cost_vel) c = 1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) if (fabsf(E.la[k]) > P.cost_rate) c = 1.0f;
    return c;
}

__device__ __forceinline__ void abuf_last(const KParams& P, const Env& E, float o[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v = opaque(E.abuf[0][j]);
#pragma unroll
        for (int r = 1; r < 4; ++r) v = (P.buf_size - 1) == r ? opaque(E.abuf[r][j]) : v;
        o[j] = v;
    }
}

// compute_history: writes out[obs_dim] = [obs_prev, A0, obs_next, A1]
template <bool NOISE>
__device__ __forceinline__ void compute_history(const KParams& P, Env& E, const float* on, float* out) {
    constexpr int OL = NOISE ? 13 : 17;
    float last[4];
    abuf_last(P, E, last);
    int o = 0;
#pragma unroll
    for (int k = 0; k < OL; ++k) out[o++] = E.obs_prev[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[o++] = E.halias0 ? last[k] : E.hact[0][k];
#pragma unroll
    for (int k = 0; k < OL; ++k) out[o++] = on[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[o++] = E.halias1 ? last[k] : E.hact[1][k];
#pragma unroll
    for (int k = 0; k < OL; ++k) E.obs_prev[k] = on[k];
    E.halias0 = E.halias1;
#pragma unroll
    for (int k = 0; k < 4; ++k) E.hact[0][k] = E.hact[1][k];
    E.halias1 = E.la_view;
#pragma unroll
    for (int k = 0; k < 4; ++k) E.hact[1][k] = E.la[k];
}

__device__ __forceinline__ int boltzmann_index(const KParams& P, float u) {
    int i = 0;
    for (int k = 0; k < P.num_levels - 1; ++k) i += ((double)u < P.tab->level_cdf[k]) ? 0 : 1;
    // cdf is non-decreasing: count of entries <= u == searchsorted(side='right')
    return i;
}

}  // namespace cf2
