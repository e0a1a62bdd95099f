// cf2sim_draws.h -- random-word sources of the env kernels: Philox streams, the LDS reset table and rows, Box-Muller normals
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf2sim_internal.h"
#include "cf2sim_rng.h"

namespace cf2 {

// Random-word sources: Rng computes Philox blocks; TableRng reads blocks a whole block of
// threads precomputed into LDS (auto-reset, see step_kernel).  Counter = (block, rng counter,
// global env id, tag).
template <class KT>
struct RngT {
    const KT& K;
    uint32_t ctr, gid, tag;
    __device__ __forceinline__ U4 block(uint32_t b) const { return philox(K, b, ctr, gid, tag); }
};
using Rng = RngT<Keys>;

// reset-time blocks (reset_env): 0-13 direct, sensor calls at 32-37 and 40-45
enum { RESET_SLOTS = 26 };
__host__ __device__ constexpr int reset_slot(uint32_t b) { return b < 14 ? (int)b : (b < 40 ? 14 + (int)b - 32 : 20 + (int)b - 40); }
__host__ __device__ constexpr uint32_t reset_block_of_slot(int s) { return s < 14 ? (uint32_t)s : (s < 20 ? 32u + (uint32_t)(s - 14) : 40u + (uint32_t)(s - 20)); }

struct TableRng {
    const uint32_t* t;      // LDS: word w of slot s at t[(s * 4 + w) * stride]
    uint32_t stride;
    __device__ __forceinline__ U4 block(uint32_t b) const {
        const uint32_t* q = t + (size_t)reset_slot(b) * 4 * stride;
        return U4{q[0], q[stride], q[2 * stride], q[3 * stride]};
    }
};

// N normals from consecutive blocks starting at b0 (pair k uses u32 2k, 2k+1)
template <int N, class G>
__device__ __forceinline__ void normals(const G& g, uint32_t b0, float (&z)[N]) {
#pragma unroll
    for (int blk = 0; blk < (N + 3) / 4; ++blk) {
        const U4 u = g.block(b0 + blk);
        float a0, a1, a2, a3;
        box_muller(u.x, u.y, a0, a1);
        if (4 * blk + 0 < N) z[4 * blk + 0] = a0;
        if (4 * blk + 1 < N) z[4 * blk + 1] = a1;
        if (4 * blk + 2 < N) {
            box_muller(u.z, u.w, a2, a3);
            z[4 * blk + 2] = a2;
            if (4 * blk + 3 < N) z[4 * blk + 3] = a3;
        }
    }
}

// The auto-reset table holds the Box-Muller outputs, not the raw words, of the word pairs the
// reset turns into normals (reset_env: blocks 4-8; its two sensor calls: blocks 32-35 and 40-43
// whole, 36 and 44 first pair).  They are transformed block-parallel while the table is drawn,
// which takes ~110 transcendentals off the one-lane-per-env reset path.
__host__ __device__ constexpr bool reset_slot_normal_xy(int s) {
    return (s >= 4 && s <= 8) || (s >= 14 && s <= 18) || (s >= 20 && s <= 24);
}
__host__ __device__ constexpr bool reset_slot_normal_zw(int s) {
    return (s >= 4 && s <= 8) || (s >= 14 && s <= 17) || (s >= 20 && s <= 23);
}
template <int N>
__device__ __forceinline__ void normals(const TableRng& g, uint32_t b0, float (&z)[N]) {
#pragma unroll
    for (int blk = 0; blk < (N + 3) / 4; ++blk) {
        const U4 u = g.block(b0 + blk);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * blk + k < N) z[4 * blk + k] = __uint_as_float(w[k]);
    }
}

// The final sensor call's six Philox blocks, drawn while the env's state is still in flight and
// parked in the lane's own LDS obs-staging row (which the observation overwrites only after the
// call): row words 0-17 are the call's 18 normals (Box-Muller already applied), 18-23 the raw words
// of its uniforms.  block(b) returns row words 4(b-b0)..+3, normals<N> the first N row words.
// STRIDE: distance between consecutive words (1: the lane's own LDS row; 64: a [word][env] table
// of the small-N kernel, where the helper waves stage the env-step's later draws)
template <uint32_t STRIDE = 1>
struct RowRng {
    const uint32_t* t;
    uint32_t b0;
    __device__ __forceinline__ U4 block(uint32_t b) const {
        const uint32_t* q = t + 4u * (b - b0) * STRIDE;
        return U4{q[0], q[STRIDE], q[2 * STRIDE], q[3 * STRIDE]};
    }
};
template <int N, uint32_t STRIDE>
__device__ __forceinline__ void normals(const RowRng<STRIDE>& g, uint32_t b0, float (&z)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) z[k] = __uint_as_float(g.t[(4u * (b0 - g.b0) + k) * STRIDE]);
}

// The small-N kernel's helper-drawn env-step randomness ([word][env] in LDS, stride 64): what the
// env-step draws from its first sensor call on in the reference-default shape (SPEC 1 with sensor
// noise), with Box-Muller already applied to the words that become normals:
//   words  0-3   OU normals of sub-step 1              (step block 2)
//   words  4-12  gyro normals of sub-step 1's call      (normals<9> at block 16: blocks 16-18)
//   words 13-30  final sensor call's 18 normals         (normals<18> at block 24: blocks 24-28)
//   words 31-36  its uniform words: block 28 .z .w, block 29 .x .y .z .w
//   words 37-45  gyro normals 6-14 of sub-step 0's call (normals_range<6, 15> at block 8: blocks 9-11;
//                the call is a full one whose held part is dead, compute_observation)
// The env wave joins the helpers' LDS barrier before that first sensor call.
enum { HD_WORDS = 46, HD_OU1 = 0, HD_GYRO1 = 4, HD_FINAL = 13, HD_GYRO0 = 37 };

// Normals LO..HI-1 of the sequence normals<N>(g, b0, .) would produce, drawing only the Philox
// blocks and Box-Muller pairs that cover them (the stream positions of all other draws are
// unchanged, so skipping dead draws is invisible to everything else).
template <int LO, int HI, class G>
__device__ __forceinline__ void normals_range(const G& g, uint32_t b0, float* z) {
#pragma unroll
    for (int blk = LO / 4; blk < (HI + 3) / 4; ++blk) {
        const U4 u = g.block(b0 + blk);
        float a[4];
        if (4 * blk + 1 >= LO && 4 * blk < HI) box_muller(u.x, u.y, a[0], a[1]);
        if (4 * blk + 3 >= LO && 4 * blk + 2 < HI) box_muller(u.z, u.w, a[2], a[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * blk + k >= LO && 4 * blk + k < HI) z[4 * blk + k] = a[k];
    }
}

// (the reset table already holds the Box-Muller outputs of its normal slots)
template <int LO, int HI>
__device__ __forceinline__ void normals_range(const TableRng& g, uint32_t b0, float* z) {
#pragma unroll
    for (int blk = LO / 4; blk < (HI + 3) / 4; ++blk) {
        const U4 u = g.block(b0 + blk);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * blk + k >= LO && 4 * blk + k < HI) z[4 * blk + k] = __uint_as_float(w[k]);
    }
}

// The small-N kernels' helper waves 1-3 draw the env-step's randomness of the HD_* layout for the
// env of their lane (d = its column of the [word][env] LDS table, stride 64), the step counter ctr
// known from the state.  Sub-step 0's gyro normals first: the env wave needs them earliest.
__device__ __forceinline__ void helper_step_draws(const Keys& K, uint32_t ctr, uint32_t gid, uint32_t wave, float* d) {
    const RngT<Keys> g{K, ctr, gid, TAG_STEP};
    auto bm4 = [&](uint32_t blk, int w) {          // 4 normals of one block -> words w..w+3
        const U4 u = g.block(blk);
        float z0, z1, z2, z3;
        box_muller(u.x, u.y, z0, z1);
        box_muller(u.z, u.w, z2, z3);
        d[(w + 0) * 64] = z0; d[(w + 1) * 64] = z1; d[(w + 2) * 64] = z2; d[(w + 3) * 64] = z3;
    };
    if (wave == 1) {
        bm4(2, HD_OU1);                             // OU of sub-step 1
        bm4(16, HD_GYRO1);                          // sub-step 1 sensor call: normals 0-8
        bm4(17, HD_GYRO1 + 4);
        const U4 u = g.block(18);
        float z0, z1;
        box_muller(u.x, u.y, z0, z1);
        d[(HD_GYRO1 + 8) * 64] = z0;
    } else if (wave == 2) {
        {
            const U4 u = g.block(9);                // sub-step 0 sensor call: normals 6-7
            float z2, z3;
            box_muller(u.z, u.w, z2, z3);
            d[(HD_GYRO0 + 0) * 64] = z2; d[(HD_GYRO0 + 1) * 64] = z3;
        }
        bm4(24, HD_FINAL);                          // final sensor call: normals 0-11
        bm4(25, HD_FINAL + 4);
        bm4(26, HD_FINAL + 8);
    } else {
        bm4(10, HD_GYRO0 + 2);                      // sub-step 0 sensor call: normals 8-11
        {
            const U4 u = g.block(11);               // normals 12-14
            float z0, z1, z2, z3;
            box_muller(u.x, u.y, z0, z1);
            box_muller(u.z, u.w, z2, z3);
            d[(HD_GYRO0 + 6) * 64] = z0; d[(HD_GYRO0 + 7) * 64] = z1; d[(HD_GYRO0 + 8) * 64] = z2;
            (void)z3;
        }
        bm4(27, HD_FINAL + 12);                     // normals 12-15
        const U4 u = g.block(28), v = g.block(29);
        float z0, z1;
        box_muller(u.x, u.y, z0, z1);               // normals 16-17, then the six uniform words
        d[(HD_FINAL + 16) * 64] = z0; d[(HD_FINAL + 17) * 64] = z1;
        d[(HD_FINAL + 18) * 64] = __uint_as_float(u.z); d[(HD_FINAL + 19) * 64] = __uint_as_float(u.w);
        d[(HD_FINAL + 20) * 64] = __uint_as_float(v.x); d[(HD_FINAL + 21) * 64] = __uint_as_float(v.y);
        d[(HD_FINAL + 22) * 64] = __uint_as_float(v.z); d[(HD_FINAL + 23) * 64] = __uint_as_float(v.w);
    }
}

}  // namespace cf2
