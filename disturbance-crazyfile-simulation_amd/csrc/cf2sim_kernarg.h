// cf2sim_kernarg.h -- kernel parameters re-read from the kernarg segment where they are used (late_*)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf2sim_internal.h"

namespace cf2 {

// The env-step's kernel parameters that only its epilogue reads (done, reward and cost thresholds
// and weights), re-read from the kernarg segment where they are used: every kernel that steps envs
// takes its KParams first, so the segment starts with them.  Through the opaque pointer the loads
// cannot be hoisted to the kernel's entry, where the compiler otherwise issues every kernarg load
// and, with ~100 scalar registers of live values across the physics, spills them to VGPR lanes
// (87 v_writelane / 279 v_readlane sites in the 262 144-env kernel).  The large-N step kernel
// re-reads the epilogue's and the final sensor call's parameters (LATEP) and the auto-reset's
// reset-only ones (reset_src<2>): 24 writelane sites left, 262 144 envs 36.3 -> 33.9 us, HJ
// 41.1 -> 39.6, 65 536 envs 14.7 -> 13.9 (profiles/r06_ab_late_params.txt); the small-N kernel,
// whose spills are few, measured +0.3 us with the epilogue part.
typedef const __attribute__((address_space(4))) KParams* KernargParams;
__device__ __forceinline__ KernargParams kernarg_params() {
    KernargParams p = (KernargParams)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
// P with the epilogue's fields re-read (done, reward, cost; the others as in P)
__device__ __forceinline__ KParams late_epilogue(const KParams& P) {
    KParams Q = P;
    const KernargParams k = kernarg_params();
    Q.pen_action = k->pen_action; Q.pen_angle = k->pen_angle; Q.pen_spin = k->pen_spin; Q.pen_term = k->pen_term;
    Q.pen_vel = k->pen_vel; Q.pen_z = k->pen_z; Q.pen_arp = k->pen_arp; Q.pen_dist = k->pen_dist;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Q.target_pos[j] = k->target_pos[j]; Q.target_rpy[j] = k->target_rpy[j]; Q.target_rate[j] = k->target_rate[j];
    }
    Q.done_rp = k->done_rp; Q.done_rate_deg = k->done_rate_deg; Q.done_zmin = k->done_zmin;
    Q.cost_xy = k->cost_xy; Q.cost_z = k->cost_z; Q.cost_rp = k->cost_rp; Q.cost_vel = k->cost_vel;
    Q.cost_rate = k->cost_rate;
    return Q;
}
// io with the per-env output pointers re-read (StepIO is the second kernel argument of every
// kernel that passes LATEP: step_kernel, collect_kernel)
typedef const __attribute__((address_space(4))) StepIO* KernargIO;
__device__ __forceinline__ StepIO late_outputs(const StepIO& io) {
    constexpr size_t off = (sizeof(KParams) + alignof(StepIO) - 1) / alignof(StepIO) * alignof(StepIO);
    KernargIO k = (KernargIO)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + off);
    asm volatile("" : "+s"(k));
    StepIO o = io;
    o.rew = k->rew; o.done = k->done; o.trunc = k->trunc; o.cost = k->cost; o.level = k->level;
    o.final_obs = k->final_obs;
    return o;
}
// every pointer of io re-read (the fused rollout derives each env-step's output slabs from them)
__device__ __forceinline__ StepIO late_io(const StepIO& io) {
    constexpr size_t off = (sizeof(KParams) + alignof(StepIO) - 1) / alignof(StepIO) * alignof(StepIO);
    KernargIO k = (KernargIO)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + off);
    asm volatile("" : "+s"(k));
    StepIO o = io;
    o.sf = k->sf; o.act = k->act; o.dstb = k->dstb; o.obs = k->obs; o.rew = k->rew; o.done = k->done;
    o.trunc = k->trunc; o.cost = k->cost; o.level = k->level; o.final_obs = k->final_obs;
    return o;
}
// P with the physics sub-step's constants re-read (the fused rollout, LATEX: its K-step loop kept
// them live across the whole loop body, spilled with the rest)
__device__ __forceinline__ KParams late_physics(const KParams& P) {
    KParams Q = P;
    const KernargParams k = kernarg_params();
    Q.time_step = k->time_step; Q.mass = k->mass; Q.ixx = k->ixx; Q.iyy = k->iyy; Q.izz = k->izz;
    Q.ft0 = k->ft0; Q.ft1 = k->ft1; Q.K = k->K; Q.B = k->B; Q.ou_sigma = k->ou_sigma;
    Q.drag_xy = k->drag_xy; Q.drag_z = k->drag_z; Q.g_world = k->g_world; Q.arm = k->arm;
    Q.prop_xy = k->prop_xy; Q.prop_z = k->prop_z; Q.prop_mass = k->prop_mass; Q.prop_inertia = k->prop_inertia;
    Q.prop_speed_gain = k->prop_speed_gain; Q.lin_damping = k->lin_damping; Q.ang_damping = k->ang_damping;
    Q.vmax = k->vmax;
    return Q;
}
// P with the reset-only fields re-read (reset_src<2>)
__device__ __forceinline__ KParams late_reset(const KParams& P) {
    KParams Q = P;
    const KernargParams k = kernarg_params();
#pragma unroll
    for (int j = 0; j < 3; ++j) Q.init_xyz[j] = k->init_xyz[j];
    Q.pos_lim = k->pos_lim; Q.angle_lim = k->angle_lim; Q.yaw_lim = k->yaw_lim; Q.vel_lim = k->vel_lim;
    Q.rate_lim = k->rate_lim; Q.yaw_rate_lim = k->yaw_rate_lim; Q.action_std = k->action_std;
    Q.motor_std = k->motor_std; Q.hover_x = k->hover_x; Q.hover_action = k->hover_action;
#pragma unroll
    for (int j = 0; j < 9; ++j) { Q.dr_lo[j] = k->dr_lo[j]; Q.dr_hi[j] = k->dr_hi[j]; }
    return Q;
}

// P with the sensor model's parameters re-read from the kernarg segment (the final sensor call of
// the large-N step kernel: the values are the same, their registers are free during the physics)
__device__ __forceinline__ KParams late_sensor(const KParams& P) {
    KParams Q = P;
    const KernargParams k = kernarg_params();
    Q.pos_std = k->pos_std; Q.pos_unif = k->pos_unif; Q.vel_std = k->vel_std; Q.rot_std = k->rot_std;
    Q.rot_unif = k->rot_unif; Q.pgd = k->pgd; Q.sbgd = k->sbgd; Q.gyro_rw = k->gyro_rw; Q.gyro_ton = k->gyro_ton;
    Q.lpf_gain = k->lpf_gain; Q.lpf_ratio = k->lpf_ratio;
    return Q;
}

// the late_* copies when L, else the argument itself (no copy of the 624-byte block: a
// conditional expression would materialise one, and that changed the small-N kernel's code)
template <bool L> __device__ __forceinline__ decltype(auto) late_epilogue_if(const KParams& P) {
    if constexpr (L) return late_epilogue(P); else return (P);
}
template <bool L> __device__ __forceinline__ decltype(auto) late_sensor_if(const KParams& P) {
    if constexpr (L) return late_sensor(P); else return (P);
}
template <bool L> __device__ __forceinline__ decltype(auto) late_physics_if(const KParams& P) {
    if constexpr (L) return late_physics(P); else return (P);
}
template <bool L> __device__ __forceinline__ decltype(auto) late_outputs_if(const StepIO& io) {
    if constexpr (L) return late_outputs(io); else return (io);
}

}  // namespace cf2
