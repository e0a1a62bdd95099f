// cf2sim_dynamics.h -- physics sub-steps (Bullet and Simple restatements) and multi-drone formations
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf2sim_internal.h"
#include "cf2sim_math.h"
#include "cf2sim_state.h"

namespace cf2 {

// ------------------------------------------------------------------------------------
// physics
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void apply_action(const KParams& P, Env& E, const float a[4], const float on[4],
                                             float f[4], float& tz) {
    float pwm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) E.la[j] = a[j];
    E.la_view = 0;
    if (P.use_latency) {
        float del[4];
        // dynamic ring index resolved with selects (no scratch)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float d = opaque(E.abuf[0][j]);
#pragma unroll
            for (int r = 1; r < 4; ++r) d = E.aidx == r ? opaque(E.abuf[r][j]) : d;
            del[j] = d;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) E.abuf[r][j] = E.aidx == r ? a[j] : E.abuf[r][j];
        E.aidx = E.aidx + 1 == P.buf_size ? 0 : E.aidx + 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) pwm[j] = 30000.0f + clampf(del[j], -1.0f, 1.0f) * 30000.0f;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) pwm[j] = 30000.0f + clampf(a[j], -1.0f, 1.0f) * 30000.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xo = E.ou[j];
        const float dx = 0.15f * (0.0f - xo) + P.ou_sigma * on[j];
        E.ou[j] = xo + dx;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float tn = pwm[j] * (1.0f / 60000.0f);      // == pwm / 60000 as compiled (see DIV_NOTE)
        float noisy;
        if (P.use_motor_dyn) {
            // x(k+1) = A x(k) + B u with A = 1 - B (agents.py:288), evaluated as x += B (u - x) on the
            // unevaluated pair x + xl (TwoSum): the recurrence then carries no fp32 rounding from
            // step to step (it dominated the drift vs the fp64 reference)
            const float rot = sqrt_fast(tn);
            const float inc = E.B[j] * ((rot - E.x[j]) - E.xl[j]);
            const float sum = E.x[j] + inc, bb = sum - E.x[j];                  // TwoSum
            const float lo = ((E.x[j] - (sum - bb)) + (inc - bb)) + E.xl[j];
            E.x[j] = sum + lo;                                                    // renormalise
            E.xl[j] = lo - (E.x[j] - sum);
            noisy = (1.0f + E.ou[j]) * (E.x[j] * E.x[j]);
        } else {
            noisy = (1.0f + E.ou[j]) * tn;
        }
        // rounded on its own (no FMA contraction into the mixer sums below): equal motor forces then
        // cancel exactly in the roll/pitch torques, as in the reference; a contracted product would
        // leave a one-sided ulp torque every sub-step (a systematic attitude drift in hover)
        f[j] = opaque(E.K[j] * clampf(noisy, 0.0f, 1.0f));
    }
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = E.k1 * f[j] + E.k0;
    tz = (-t[0] + t[1] - t[2] + t[3]);
}

// GE: calculate_ground_effect on (physics_kernel only: the reference's envs never enable it, and the
// env-step kernels keep their code free of the branch)
template <bool GE = false>
__device__ __forceinline__ void bullet_substep(const KParams& P, Env& E, const float a[4], const float d[3],
                                               const float on[4], bool first_after_reset, float dw = 0.0f) {
    float xprev[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xprev[j] = E.x[j];
    float f[4], tz;
    apply_action(P, E, a, on, f, tz);
    const M3 R = rotmat(E.q);
    float ssum = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float rpm = E.x[j] * E.x[j] * 25000.0f;
        ssum += 2.0f * 3.141592653589793f * rpm * (1.0f / 60.0f);     // DIV_NOTE
    }
    const float dl[3] = {-1.0f * P.drag_xy * ssum * E.v[0], -1.0f * P.drag_xy * ssum * E.v[1], -1.0f * P.drag_z * ssum * E.v[2]};
    float drag1[3], dragw[3];
    mv(R, dl, drag1);
    mv(R, drag1, dragw);
    const float L = P.prop_xy;
    const float mp = P.prop_mass, Ip = P.prop_inertia, Lz = P.prop_z;
    if (GE && fabsf(E.rpy[0]) < 1.5707963267948966f && fabsf(E.rpy[1]) < 1.5707963267948966f) {
        // BasePhysics.calculate_ground_effect (physics.py:27-58): extra thrust at each prop from its
        // height z_i = (p + R o_i)_z (getLinkStates), clipped at GND_EFF_H_CLIP; added to the prop
        // forces (apply_motor_forces, physics.py:243-246), not to the yaw torque.  rpy: the last readback.
        const float ox[4] = {L, -L, -L, L}, oy[4] = {-L, -L, L, L};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float z = fmaxf(E.p[2] + (R.m[6] * ox[j] + R.m[7] * oy[j] + R.m[8] * Lz), P.gnd_eff_h_clip);
            const float rr = P.prop_radius * rcp(4.0f * z);
            f[j] = opaque(f[j] + f[j] * P.gnd_eff_coeff * (rr * rr));
        }
    }
    float tb[3];
    tb[0] = L * (-f[0] - f[1] + f[2] + f[3]) + d[0];
    tb[1] = L * (-f[0] + f[1] + f[2] - f[3]) + d[1];
    tb[2] = tz;
    const float fsum = f[0] + f[1] + f[2] + f[3];
    const float mtot = E.m + 4.0f * mp;
    float Fw[3];
    const float fz = fsum - dw;      // downwash of formation mates: -z of the body, at the COM
    Fw[0] = R.m[2] * fz + dragw[0];
    Fw[1] = R.m[5] * fz + dragw[1];
    Fw[2] = R.m[8] * fz + dragw[2] - P.g_world * mtot;
    float wb[3], vb[3];
    mtv(R, E.w, wb);
    mtv(R, E.v, vb);
    const float wn = norm3(wb), vn = norm3(vb);
    float Ic[3];
    Ic[0] = E.J[0] + 4.0f * Ip + 4.0f * mp * (L * L + Lz * Lz);
    Ic[1] = E.J[1] + 4.0f * Ip + 4.0f * mp * (L * L + Lz * Lz);
    Ic[2] = E.J[2] + 4.0f * Ip + 4.0f * mp * (L * L + L * L);
    const float kq = P.prop_speed_gain;
    const float sp_old = first_after_reset ? 0.0f : kq * (-xprev[0] + xprev[1] - xprev[2] + xprev[3]);
    const float sp_new = kq * (-E.x[0] + E.x[1] - E.x[2] + E.x[3]);
    const float h_old = Ip * sp_old;
    const float Iw[3] = {Ic[0] * wb[0], Ic[1] * wb[1], Ic[2] * wb[2] + h_old};
    const float gyro[3] = {wb[1] * Iw[2] - wb[2] * Iw[1], wb[2] * Iw[0] - wb[0] * Iw[2], wb[0] * Iw[1] - wb[1] * Iw[0]};
    const float dampa = P.ang_damping * (1.0f + wn);
    const float tdamp[3] = {E.J[0] * wb[0] * dampa, E.J[1] * wb[1] * dampa, E.J[2] * wb[2] * dampa};
    float pd[3] = {0.0f, 0.0f, 0.0f};
    {
        const float ax[4] = {-1.0f, 1.0f, -1.0f, 1.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float qd = first_after_reset ? 0.0f : kq * xprev[j];
            const float wp[3] = {wb[0], wb[1], wb[2] + ax[j] * qd};
            const float k = Ip * P.ang_damping * (1.0f + norm3(wp));
            pd[0] += k * wp[0]; pd[1] += k * wp[1]; pd[2] += k * wp[2];
        }
    }
    const float dt = E.dt;
    float wdot_b[3];
    wdot_b[0] = (tb[0] - gyro[0] - tdamp[0] - pd[0]) * rcp(Ic[0]);
    wdot_b[1] = (tb[1] - gyro[1] - tdamp[1] - pd[1]) * rcp(Ic[1]);
    wdot_b[2] = (tb[2] - gyro[2] - tdamp[2] - pd[2] - Ip * (sp_new - sp_old) * rcp(dt)) * rcp(Ic[2]);
    const float imtot = rcp(mtot);
    const float dampl = P.lin_damping * (1.0f + vn) * E.m * imtot;
    float vdot_w[3], wdot_w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vdot_w[k] = Fw[k] * imtot - dampl * E.v[k];
    mv(R, wdot_b, wdot_w);
    const float vmax = P.vmax;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        E.w[k] = clampf(E.w[k] + wdot_w[k] * dt, -vmax, vmax);
        E.v[k] = clampf(E.v[k] + vdot_w[k] * dt, -vmax, vmax);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) E.p[k] += dt * E.v[k];
    {
        float ang = norm3(E.w);
        ang = ang * dt > 0.7853981633974483f ? 0.7853981633974483f * rcp(dt) : ang;
        // half-angle h = ang*dt/2 <= pi/8 after the clamp: odd/even Taylor polynomials are exact to
        // fp32 there (truncation < 3e-13), cheaper and more accurate than the hardware sin/cos
        const float h = 0.5f * ang * dt, h2 = h * h;
        const float sin_h = h * (1.0f + h2 * (-1.6666667e-1f + h2 * (8.3333333e-3f + h2 * (-1.9841270e-4f + h2 * 2.7557319e-6f))));
        const float cw = 1.0f + h2 * (-0.5f + h2 * (4.1666668e-2f + h2 * (-1.3888889e-3f + h2 * (2.4801587e-5f - h2 * 2.7557319e-7f))));
        const float s = ang < 0.001f ? 0.5f * dt - (dt * dt * dt) * 0.020833333333f * ang * ang : sin_h * rcp(ang);
        const float axs[3] = {E.w[0] * s, E.w[1] * s, E.w[2] * s};
        const float qx = E.q[0], qy = E.q[1], qz = E.q[2], qw = E.q[3];
        const float nx = cw * qx + axs[0] * qw + axs[1] * qz - axs[2] * qy;
        const float ny = cw * qy + axs[1] * qw + axs[2] * qx - axs[0] * qz;
        const float nz = cw * qz + axs[2] * qw + axs[0] * qy - axs[1] * qx;
        const float nw = cw * qw - axs[0] * qx - axs[1] * qy - axs[2] * qz;
        const float il = rsq(nx * nx + ny * ny + nz * nz + nw * nw);
        E.q[0] = nx * il; E.q[1] = ny * il; E.q[2] = nz * il; E.q[3] = nw * il;
    }
    // update_information
    euler_from_quat(E.q, E.rpy);
    const M3 Rn = rotmat(E.q);
    mtv(Rn, E.w, E.wb);
}

__device__ __forceinline__ void simple_substep(const KParams& P, Env& E, const float a[4], const float on[4]) {
    float f[4], tz;
    apply_action(P, E, a, on, f, tz);
    const M3 R = rotmat(E.q);
    const float fsum = f[0] + f[1] + f[2] + f[3];
    const float Fw[3] = {R.m[2] * fsum - 0.0f * E.m, R.m[5] * fsum - 0.0f * E.m, R.m[8] * fsum - P.g_world * E.m};
    const float tx = (-f[0] - f[1] + f[2] + f[3]) * P.arm / sqrtf(2.0f);
    const float ty = (-f[0] + f[1] + f[2] - f[3]) * P.arm / sqrtf(2.0f);
    float* w = E.wb;
    const float Jw[3] = {E.J[0] * w[0], E.J[1] * w[1], E.J[2] * w[2]};
    const float cr[3] = {w[1] * Jw[2] - w[2] * Jw[1], w[2] * Jw[0] - w[0] * Jw[2], w[0] * Jw[1] - w[1] * Jw[0]};
    const float t[3] = {tx - cr[0], ty - cr[1], tz - cr[2]};
    const float wdd[3] = {rcp(E.J[0]) * t[0], rcp(E.J[1]) * t[1], rcp(E.J[2]) * t[2]};
    const float im = rcp(E.m);
    const float acc[3] = {Fw[0] * im, Fw[1] * im, Fw[2] * im};
    const float dt = E.dt;
#pragma unroll
    for (int k = 0; k < 3; ++k) E.v[k] += dt * acc[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) E.wb[k] += dt * wdd[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) E.p[k] += dt * E.v[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) E.rpy[k] += dt * E.wb[k];
    quat_from_euler(E.rpy, E.q);
    if (E.p[2] < 0.0f) E.p[2] = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) E.w[k] = E.wb[k];   // simple mode stores body rates in F_OMEGA
}

// ------------------------------------------------------------------------------------
// multi-drone formations (no reference implementation): the drones of a
// group are consecutive lanes of one wave, so mates' positions are wave shuffles
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void formation_offset(const KParams& P, uint32_t member, float off[3]) {
    const int ncol = (P.num_drones + 1) / 2;
    off[0] = P.num_drones > 1 ? ((float)(int)(member / 2) - (float)(ncol - 1) * 0.5f) * P.formation_dx : 0.0f;
    off[1] = 0.0f;
    off[2] = P.num_drones > 1 ? (float)(int)(member % 2) * P.formation_dz : 0.0f;
}
// gym-pybullet-drones BaseAviary._downwash summed over the mates above this drone
__device__ __forceinline__ float downwash(const KParams& P, const float p[3], uint32_t member) {
    float F = 0.0f;
    for (int j = 0; j < P.num_drones; ++j) {
        const float qx = __shfl(p[0], j, P.num_drones), qy = __shfl(p[1], j, P.num_drones),
                    qz = __shfl(p[2], j, P.num_drones);
        const float dz = qz - p[2], dx = qx - p[0], dy = qy - p[1];
        const float dxy = sqrt_fast(dx * dx + dy * dy);
        if ((uint32_t)j != member && dz > 0.0f && dxy < 10.0f) {
            const float rr = P.prop_radius * rcp(4.0f * dz);
            const float alpha = P.dw_coeff[0] * rr * rr;
            const float q = dxy * rcp(P.dw_coeff[1] * dz + P.dw_coeff[2]);
            F += alpha * __builtin_amdgcn_exp2f(-0.72134752044448170f * q * q);   // exp(-q^2/2)
        }
    }
    return F;
}

}  // namespace cf2
