// cf2sim_math.h -- fp32 maths helpers of the env kernels: rotations, short-range elementary functions
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cf2 {

// ------------------------------------------------------------------------------------
// rotation helpers (PyBullet C-API semantics)
// ------------------------------------------------------------------------------------
// DIV_NOTE: a division by a constant, x / c, is compiled (fp32, -fno-hip-fp32-correctly-rounded-
// divide-sqrt) as frexp(x), mantissa * rn(1 / c) scaled to [1, 2), ldexp: five VALU, and for every
// normal x bit-identical to x * rn(1 / c) (scaling by a power of two commutes with rounding), which
// is one.  The env-step divides by constants 19 times (PWM, rpm, the done test): written as products.
// v_rcp_f32 / v_rsq_f32 (1 ulp) for well-scaled operands (no denormal pre-scaling)
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }

struct M3 { float m[9]; };

__device__ __forceinline__ M3 rotmat(const float q[4]) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float d = x * x + y * y + z * z + w * w;
    const float s = 2.0f * rcp(d);
    const float xs = x * s, ys = y * s, zs = z * s;
    const float wx = w * xs, wy = w * ys, wz = w * zs;
    const float xx = x * xs, xy = x * ys, xz = x * zs;
    const float yy = y * ys, yz = y * zs, zz = z * zs;
    M3 r;
    r.m[0] = 1.0f - (yy + zz); r.m[1] = xy - wz;          r.m[2] = xz + wy;
    r.m[3] = xy + wz;          r.m[4] = 1.0f - (xx + zz); r.m[5] = yz - wx;
    r.m[6] = xz - wy;          r.m[7] = yz + wx;          r.m[8] = 1.0f - (xx + yy);
    return r;
}
__device__ __forceinline__ void mv(const M3& R, const float v[3], float o[3]) {
    o[0] = R.m[0] * v[0] + R.m[1] * v[1] + R.m[2] * v[2];
    o[1] = R.m[3] * v[0] + R.m[4] * v[1] + R.m[5] * v[2];
    o[2] = R.m[6] * v[0] + R.m[7] * v[1] + R.m[8] * v[2];
}
__device__ __forceinline__ void mtv(const M3& R, const float v[3], float o[3]) {
    o[0] = R.m[0] * v[0] + R.m[3] * v[1] + R.m[6] * v[2];
    o[1] = R.m[1] * v[0] + R.m[4] * v[1] + R.m[7] * v[2];
    o[2] = R.m[2] * v[0] + R.m[5] * v[1] + R.m[8] * v[2];
}
// v_sqrt_f32 without the denormal pre-scaling sqrtf adds (6 instructions -> 1): the same result
// for every normal operand; a denormal operand (|v| < 1e-19) gives 0
__device__ __forceinline__ float sqrt_fast(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float norm3(const float v[3]) { return sqrt_fast(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
// clip(x, lo, hi) for lo <= hi as one v_med3_f32 (identical to the compare form for non-NaN x)
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }
// Makes a register value opaque to the optimiser.  Used before data-dependent selects among
// Env fields: otherwise InstCombine turns select(c, load p, load q) chains into a load of a
// select of pointers, SROA can no longer promote the Env struct and it lands in scratch.
__device__ __forceinline__ float opaque(float x) { asm("" : "+v"(x)); return x; }

// ---- short-range elementary functions (VALU polynomials instead of the ocml library paths,
// whose general range reduction costs ~100 instructions each).  Errors are a few fp32 ulp.
// sin and cos of x: Cody-Waite reduction by pi/2 (3-part constant, exact for |x| < ~1e4), then
// degree-11/12 Taylor polynomials on [-pi/4, pi/4] (truncation < 2e-9)
__device__ __forceinline__ void sincos_fast(float x, float& s, float& c) {
    const float k = __builtin_rintf(x * 0.63661977236758134f);
    float r = __builtin_fmaf(k, -1.5707963705062866f, x);
    r = __builtin_fmaf(k, 4.3711388286737929e-08f, r);
    r = __builtin_fmaf(k, 1.7151245100059206e-15f, r);
    const float r2 = r * r;
    const float sr = r * (1.0f + r2 * (-1.6666667e-1f + r2 * (8.3333333e-3f + r2 * (-1.9841270e-4f + r2 * (2.7557319e-6f - r2 * 2.5052108e-8f)))));
    const float cr = 1.0f + r2 * (-0.5f + r2 * (4.1666668e-2f + r2 * (-1.3888889e-3f + r2 * (2.4801587e-5f + r2 * (-2.7557319e-7f + r2 * 2.0876757e-9f)))));
    const int q = (int)k & 3;
    const float ss = (q & 1) ? cr : sr, cc = (q & 1) ? sr : cr;
    s = (q & 2) ? -ss : ss;
    c = ((q + 1) & 2) ? -cc : cc;
}
// atan2 (Cephes atanf kernel on the reduced ratio min/max in [0, 1], reduced again about 1)
__device__ __forceinline__ float atan2_fast(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float t = mx > 0.0f ? mn * rcp(mx) : 0.0f;
    const bool red = t > 0.41421356237309503f;
    const float z = red ? (t - 1.0f) * rcp(t + 1.0f) : t;
    const float z2 = z * z;
    float r = (((8.05374449538e-2f * z2 - 1.38776856032e-1f) * z2 + 1.99777106478e-1f) * z2 - 3.33329491539e-1f) * z2 * z + z;
    r = red ? r + 0.78539816339744831f : r;
    r = ay > ax ? 1.5707963267948966f - r : r;
    r = x < 0.0f ? 3.1415926535897932f - r : r;
    return __builtin_copysignf(r, y);
}
__device__ __forceinline__ float asin_fast(float x) {
    return atan2_fast(x, sqrt_fast(fmaxf(0.0f, (1.0f - x) * (1.0f + x))));
}

__device__ __forceinline__ void quat_from_euler(const float e[3], float q[4]) {
    const float phi = e[0] * 0.5f, the = e[1] * 0.5f, psi = e[2] * 0.5f;
    float sp, cp, st, ct, ss, cs;
    sincos_fast(phi, sp, cp);
    sincos_fast(the, st, ct);
    sincos_fast(psi, ss, cs);
    const float x = sp * ct * cs - cp * st * ss;
    const float y = cp * st * cs + sp * ct * ss;
    const float z = cp * ct * ss - sp * st * cs;
    const float w = cp * ct * cs + sp * st * ss;
    const float il = rsq(x * x + y * y + z * z + w * w);
    q[0] = x * il; q[1] = y * il; q[2] = z * il; q[3] = w * il;
}
// the observation's quaternion of the noisy rpy (sensors.py): sin/cos on the transcendental unit
// (v_sin/v_cos take revolutions), 3 muls + 6 quarter-rate ops instead of ~75 polynomial VALU ops
__device__ __forceinline__ void quat_from_euler_obs(const float e[3], float q[4]) {
    constexpr float inv4pi = 0.079577471545947668f;     // half angle in revolutions: e / 2 / (2 pi)
    const float phi = e[0] * inv4pi, the = e[1] * inv4pi, psi = e[2] * inv4pi;
    const float sp = __builtin_amdgcn_sinf(phi), cp = __builtin_amdgcn_cosf(phi);
    const float st = __builtin_amdgcn_sinf(the), ct = __builtin_amdgcn_cosf(the);
    const float ss = __builtin_amdgcn_sinf(psi), cs = __builtin_amdgcn_cosf(psi);
    const float x = sp * ct * cs - cp * st * ss;
    const float y = cp * st * cs + sp * ct * ss;
    const float z = cp * ct * ss - sp * st * cs;
    const float w = cp * ct * cs + sp * st * ss;
    const float il = rsq(x * x + y * y + z * z + w * w);
    q[0] = x * il; q[1] = y * il; q[2] = z * il; q[3] = w * il;
}
__device__ __forceinline__ void euler_from_quat(const float q[4], float e[3]) {
    const float sqx = q[0] * q[0], sqy = q[1] * q[1], sqz = q[2] * q[2], squ = q[3] * q[3];
    const float sarg = -2.0f * (q[0] * q[2] - q[3] * q[1]);
    // branch-free form of the three cases (gimbal lock at sarg <= -0.99999 / >= 0.99999): the
    // atan2 of the yaw takes case-selected arguments, so each function is evaluated once
    const bool lo = sarg <= -0.99999f, hi = sarg >= 0.99999f, mid = !(lo || hi);
    const float e0 = atan2_fast(2.0f * (q[1] * q[2] + q[3] * q[0]), squ - sqx - sqy + sqz);
    const float e1 = asin_fast(fminf(fmaxf(sarg, -1.0f), 1.0f));
    const float y2 = mid ? 2.0f * (q[0] * q[1] + q[3] * q[2]) : (lo ? q[0] : -q[0]);
    const float x2 = mid ? squ + sqx - sqy - sqz : (lo ? -q[1] : q[1]);
    const float e2 = atan2_fast(y2, x2);
    e[0] = mid ? e0 : 0.0f;
    e[1] = mid ? e1 : (lo ? -0.5f * 3.141592653589793f : 0.5f * 3.141592653589793f);
    e[2] = mid ? e2 : 2.0f * e2;
}
__device__ __forceinline__ void quat2euler(const float q[4], float e[3]) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float t0 = 2.0f * (w * x + y * z);
    const float t1 = 1.0f - 2.0f * (x * x + y * y);
    e[0] = atan2f(t0, t1);
    float t2 = 2.0f * (w * y - z * x);
    t2 = t2 > 1.0f ? 1.0f : t2;
    t2 = t2 < -1.0f ? -1.0f : t2;
    e[1] = asinf(t2);
    const float t3 = 2.0f * (w * z + x * y);
    const float t4 = 1.0f - 2.0f * (y * y + z * z);
    e[2] = atan2f(t3, t4);
}

}  // namespace cf2
