// cf2sim_ppo.hip -- loss and gradient of the PPO update (compute_loss_pi without
// the entropy term, and the critic's mean squared error), one fused launch per network plus a merge
// launch.  No env-step code here.
//
// Both kernels read the flat weight block (PolicyLayout<D>, cf2sim_policy.h; what the optimiser owns)
// and write the gradient back in that layout.  A wave works through 16-row tiles.  Everything of a
// tile between the observation load and the gradient accumulators stays in registers or LDS:
//
//   forward   the transposed formulation of the collect path's forward: H^T[neuron][row] on
//             v_mfma_f32_16x16x4_f32, the weights as the A operand (from the block's zero-padded LDS
//             copy), the activations as the B operand.  An accumulator tile (lane & 15 = row,
//             registers = neurons 16t + 4g + i) is the next layer's B operand as it stands, with the
//             k-steps taken in the permuted order (t, i).  Layer 3 (4 or 1 outputs) runs on the VALU:
//             16 fmaf per output and lane, then a butterfly over the four lane groups.
//   head      per row: log-probability, ratio, clipped surrogate and its derivative (policy), or the
//             squared error (value); the fp64 sums of the summary stay in the lane.
//   backward  dZ^T of a layer is again an accumulator-layout tile, so dH1^T = W2 dZ2^T takes it as the
//             B operand with no data movement (A = W2 read transposed from the same LDS copy).
//   gradient  dW[in][out] = sum over rows act[row][in] dZ[row][out] is a GEMM whose k dimension is the
//             rows: both operands go through the wave's LDS staging tile ([row][neuron]) and come
//             back as A[in][row], B[row][out], 4 k-steps per 16 rows.  The accumulators (dW1: 3 x 4
//             tiles, dW2: 4 x 4 tiles of 4 registers) live in the wave's registers for the whole
//             kernel.  Bias and layer-3 gradients are per-lane sums, reduced over the 16 row lanes
//             once at the end.
//
// The next tile's observations and the head's row inputs are loaded before the layers and land
// under them (one wave per SIMD has nothing else to hide a global load behind).
//
// Reduction: the four waves of a block add their accumulators into LDS in wave order, the block
// writes one partial gradient and one partial summary to scratch, and ppo_merge_kernel sums the
// partials in block-index order in fp64, divides by m and rounds once.  No atomics; the geometry
// depends on m only, so the same input gives the same bits.  The rank-partial calls of the
// data-parallel updates end in ppo_partial_merge_kernel instead: the same sums, not divided and not
// rounded, as one block of doubles that cf2_ppo_reduce (cf2sim_reduce.hip) merges across ranks.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cf2sim.h"
#include "cf2sim_internal.h"
#include "cf2sim_policy.h"

namespace cf2 {

constexpr int PPO_BLOCK = 256, PPO_WAVES = PPO_BLOCK / 64;
constexpr uint32_t PPO_MAX_BLOCKS = 512;      // scratch is sized for at most this many partials
constexpr int PPO_SUM = 8;                    // doubles per partial summary
// LDS row strides (floats): odd, so that the two lane groups of a 32-lane half (rows k, k + 1 or
// neurons 4 apart) fall on banks at most 2-way shared
constexpr int PPO_WS = 65, PPO_AS = 65, PPO_ZS = 49;

template <int D, bool PI>
struct PpoNet {
    using L = PolicyLayout<D>;
    static constexpr int H = PI ? 50 : 64, NO = PI ? 4 : 1;
    static constexpr int BASE = PI ? L::P_W1 : L::V_W1;                  // the slice's start in the flat block
    static constexpr int W1 = 0, B1 = W1 + D * H, W2 = B1 + H, B2 = W2 + H * H, W3 = B2 + H, B3 = W3 + H * NO,
                         NPAR = B3 + NO;
    static constexpr int KS1 = (D + 3) / 4, KP1 = 4 * KS1, KT1 = (D + 15) / 16;
    // LDS map (floats)
    static constexpr int S_W1 = 0, S_W2 = S_W1 + KP1 * PPO_WS, S_W3 = S_W2 + 64 * PPO_WS, S_B1 = S_W3 + 64 * 4,
                         S_B2 = S_B1 + 64, S_B3 = S_B2 + 64, S_MEAN = S_B3 + 4, S_SCALE = S_MEAN + 48,
                         S_WAVE = S_SCALE + 48;
    static constexpr int WAVE_Z = 0, WAVE_ACT = 16 * PPO_ZS, WAVE_DZ = WAVE_ACT + 16 * PPO_AS,
                         WAVE_FLOATS = WAVE_DZ + 16 * PPO_AS;
    static constexpr int LDS_FLOATS = S_WAVE + PPO_WAVES * WAVE_FLOATS;
    static_assert(NPAR == (PI ? L::P_LOGSTD - L::P_W1 : L::O_MEAN - L::V_W1), "slice of the flat block");
    static_assert(NPAR <= S_WAVE, "the block's gradient sum re-uses the weight area");
    static_assert(16 * KT1 <= 48 && 16 * KT1 < PPO_ZS + 1, "observation tile width");
};

struct PpoArgs {
    const float* W;
    const float* obs;
    const float* act;
    const float* logp_old;
    const float* adv;            // policy: advantages; value: targets
    const uint32_t* idx;
    const double* adv_moments;
    const float* mu_old;
    float* mu_out;
    float* logp_out;             // policy: logp [m]; value: V [m]
    double* part_sum;            // [blocks][PPO_SUM]
    float* part_grad;            // [blocks][NPAR]
    uint32_t n, m;
    float clip;
    const uint32_t* gate;        // optional: a non-zero word makes the launch return at once, nothing written
};

// LDS written by some lanes of the wave and read by others: DS instructions of one wave execute in
// order, the fences keep the compiler from moving an access across
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool PI>
__device__ __forceinline__ float ppo_act(float x) {
    if constexpr (PI) return relu(x);
    else return tanhf(x);
}
// d act / d pre-activation from the activation's value (ReLU: 0 at pre-activation <= 0)
template <bool PI>
__device__ __forceinline__ float ppo_dact(float h, float d) {
    if constexpr (PI) return h > 0.0f ? d : 0.0f;
    else return d * fmaf(-h, h, 1.0f);
}

// sum over the 16 row lanes of a lane group; every lane gets the same bits
__device__ __forceinline__ float sum_rows(float x) {
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) x += __shfl_xor(x, d);
    return x;
}

// P members in one launch (cf2_ppo_*_grad_pop; ppo_kernel<D, PI, GRAD, true>): `base` holds member 0's
// pointers, member k's lie k strides (in elements) further on.  Block b serves member b / bpm as that
// member's block b % bpm of bpm = ppo_blocks(m), the grid the member has alone, through the one kernel
// body: the same expressions, tile loop, LDS map and reduction order, hence the same bits.  The gate
// word of member k is gate[4 k]: a gated member's blocks return at once, the others never look at it.
struct PpoPopArgs {
    PpoArgs base;                // n, m shared; clip unused; part_sum, part_grad: member 0's slice of the scratch
    const float* clip;           // [P]
    size_t s_w, s_obs, s_act, s_logp_old, s_adv, s_idx, s_mu_old, s_mu_out, s_logp_out;
    size_t s_scratch;            // bytes between the members' scratch slices
    uint32_t bpm;
};

__device__ __forceinline__ PpoArgs ppo_member_args(const PpoPopArgs& p, const uint32_t k) {
    PpoArgs a = p.base;
    a.W += k * p.s_w;
    a.obs += k * p.s_obs;
    if (a.act) a.act += k * p.s_act;
    if (a.logp_old) a.logp_old += k * p.s_logp_old;
    a.adv += k * p.s_adv;
    if (a.idx) a.idx += k * p.s_idx;
    if (a.adv_moments) a.adv_moments += 2u * (size_t)k;
    if (a.mu_old) a.mu_old += k * p.s_mu_old;
    if (a.mu_out) a.mu_out += k * p.s_mu_out;
    if (a.logp_out) a.logp_out += k * p.s_logp_out;
    a.part_sum = reinterpret_cast<double*>(reinterpret_cast<char*>(a.part_sum) + k * p.s_scratch);
    a.part_grad = reinterpret_cast<float*>(reinterpret_cast<char*>(a.part_grad) + k * p.s_scratch);
    if (p.clip) a.clip = p.clip[k];
    if (a.gate) a.gate += 4u * (size_t)k;
    return a;
}

// What a kernel instance is launched with, the member's PpoArgs and the block geometry its body
// sees.  The body stays in the __global__ function, with the stand-alone instance reading its own
// kernel argument, blockIdx and gridDim as before: moved into a __device__ function that two kernels
// call, the policy-gradient instances spilled (24 and 92 bytes per lane) and every instance's code
// changed; this way the stand-alone instances' code is unchanged byte for byte.
template <bool POP> struct PpoKernelArgs { using type = PpoArgs; };
template <> struct PpoKernelArgs<true> { using type = PpoPopArgs; };
__device__ __forceinline__ const PpoArgs& ppo_args_of(const PpoArgs& a) { return a; }
__device__ __forceinline__ PpoArgs ppo_args_of(const PpoPopArgs& p) { return ppo_member_args(p, blockIdx.x / p.bpm); }
__device__ __forceinline__ uint32_t ppo_block_of(const PpoArgs&) { return blockIdx.x; }
__device__ __forceinline__ uint32_t ppo_block_of(const PpoPopArgs& p) { return blockIdx.x % p.bpm; }
__device__ __forceinline__ uint32_t ppo_nblocks_of(const PpoArgs&) { return gridDim.x; }
__device__ __forceinline__ uint32_t ppo_nblocks_of(const PpoPopArgs& p) { return p.bpm; }

// POP = false: one learner, block blockIdx.x of gridDim.x.  POP = true: P members, this block being
// block ppo_block_of(ka) of its member's ppo_nblocks_of(ka).
template <int D, bool PI, bool GRAD, bool POP = false>
__global__ void __launch_bounds__(PPO_BLOCK) ppo_kernel(const typename PpoKernelArgs<POP>::type ka) {
    using N = PpoNet<D, PI>;
    using L = PolicyLayout<D>;
    const PpoArgs& a = ppo_args_of(ka);
    constexpr int H = N::H, NO = N::NO, WS = PPO_WS, AS = PPO_AS, ZS = PPO_ZS;
    if (a.gate && *a.gate != 0u) return;          // the same word for every block: this launch only reads it
    __shared__ __attribute__((aligned(16))) float lds[N::LDS_FLOATS];
    __shared__ double sred[PPO_WAVES][PPO_SUM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    float* W1s = lds + N::S_W1;
    float* W2s = lds + N::S_W2;
    float* W3s = lds + N::S_W3;
    float* b1s = lds + N::S_B1;
    float* b2s = lds + N::S_B2;
    float* b3s = lds + N::S_B3;
    float* means = lds + N::S_MEAN;
    float* scales = lds + N::S_SCALE;
    float* Z = lds + N::S_WAVE + wave * N::WAVE_FLOATS + N::WAVE_Z;
    float* ACT = lds + N::S_WAVE + wave * N::WAVE_FLOATS + N::WAVE_ACT;
    float* DZ = lds + N::S_WAVE + wave * N::WAVE_FLOATS + N::WAVE_DZ;

    // ---- the net's weights, zero-padded to 64 neurons per layer
    const float* Wn = a.W + N::BASE;
    for (int e = tid; e < N::KP1 * 64; e += PPO_BLOCK) {
        const int k = e >> 6, n = e & 63;
        W1s[k * WS + n] = (k < D && n < H) ? Wn[N::W1 + k * H + n] : 0.0f;
    }
    for (int e = tid; e < 64 * 64; e += PPO_BLOCK) {
        const int k = e >> 6, n = e & 63;
        W2s[k * WS + n] = (k < H && n < H) ? Wn[N::W2 + k * H + n] : 0.0f;
    }
    {
        const int k = tid >> 2, o = tid & 3;
        W3s[tid] = (k < H && o < NO) ? Wn[N::W3 + k * NO + o] : 0.0f;
    }
    if (tid < 64) {
        b1s[tid] = tid < H ? Wn[N::B1 + tid] : 0.0f;
        b2s[tid] = tid < H ? Wn[N::B2 + tid] : 0.0f;
        if (tid < 4) b3s[tid] = tid < NO ? Wn[N::B3 + tid] : 0.0f;
        if (tid < 48) {
            means[tid] = tid < D ? a.W[L::O_MEAN + tid] : 0.0f;
            scales[tid] = tid < D ? a.W[L::O_SCALE + tid] : 0.0f;
        }
    }
    for (int e = lane; e < 16 * ZS; e += 64) Z[e] = 0.0f;        // the columns past D stay 0
    __syncthreads();

    // ---- per-lane constants
    float ls[4] = {0.0f, 0.0f, 0.0f, 0.0f}, inv_var[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double inv_sd[4] = {0.0, 0.0, 0.0, 0.0};
    double adv_mean = 0.0, adv_den = 1.0;
    if constexpr (PI) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ls[k] = a.W[L::P_LOGSTD + k];
            inv_sd[k] = exp(-(double)ls[k]);
            inv_var[k] = (float)exp(-2.0 * (double)ls[k]);
        }
        if (a.adv_moments) {
            adv_mean = a.adv_moments[0];
            adv_den = sqrt(a.adv_moments[1] / (double)a.n) + 1e-8;
        }
    }
    const float clip_lo = 1.0f - a.clip, clip_hi = 1.0f + a.clip;

    // ---- accumulators
    f4v acc1[GRAD ? N::KT1 : 1][4], acc2[4][4];
    float w3acc[4][4][NO], b1acc[4][4], b2acc[4][4], b3acc[NO];
    if constexpr (GRAD) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int kt = 0; kt < N::KT1; ++kt) acc1[kt][t] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) acc2[kt][t] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                b1acc[t][i] = 0.0f;
                b2acc[t][i] = 0.0f;
#pragma unroll
                for (int o = 0; o < NO; ++o) w3acc[t][i][o] = 0.0f;
            }
        }
#pragma unroll
        for (int o = 0; o < NO; ++o) b3acc[o] = 0.0f;
    }
    double S[5] = {0.0, 0.0, 0.0, 0.0, 0.0};

    const uint32_t ntiles = (a.m + 15u) / 16u, nwaves = ppo_nblocks_of(ka) * PPO_WAVES;
    // the row of position 16 tile + c; a position past m reads row m - 1 and contributes nothing
    auto row_of = [&](uint32_t tile) {
        const uint32_t jc = __builtin_elementwise_min(tile * 16u + (uint32_t)c, a.m - 1u);
        return a.idx ? __builtin_elementwise_min(a.idx[jc], a.n - 1u) : jc;
    };
    // the tile's 16 D observation words, 64 per load, raw; element e of the tile is lane e % 64's
    constexpr int ZIT = (16 * D + 63) / 64;
    float xr[ZIT];
    auto load_obs = [&](uint32_t row) {
#pragma unroll
        for (int it = 0; it < ZIT; ++it) {
            const int e = it * 64 + lane, ee = e < 16 * D ? e : 16 * D - 1;
            const int r = ee / D, k = ee - r * D;
            xr[it] = a.obs[(size_t)__shfl(row, r) * D + k];
        }
    };
    uint32_t tile = ppo_block_of(ka) * PPO_WAVES + wave;
    uint32_t row = row_of(tile < ntiles ? tile : ntiles - 1u);
    load_obs(row);
    for (; tile < ntiles; tile += nwaves) {
        const uint32_t j = tile * 16u + (uint32_t)c;
        const bool valid = j < a.m;
        // standardised observations -> Z[row of the tile][input]
#pragma unroll
        for (int it = 0; it < ZIT; ++it) {
            const int e = it * 64 + lane, ee = e < 16 * D ? e : 16 * D - 1;
            const int r = ee / D, k = ee - r * D;
            if (e < 16 * D) Z[r * ZS + k] = (xr[it] - means[k]) * scales[k];
        }
        wave_lds_sync();
        // the head's row inputs, and the next tile's observations, stay in flight under the layers
        float4 av = {0.0f, 0.0f, 0.0f, 0.0f}, mo = {0.0f, 0.0f, 0.0f, 0.0f};
        float lpo = 0.0f;
        if constexpr (PI) {
            av = reinterpret_cast<const float4*>(a.act)[row];
            lpo = a.logp_old[row];
            if (a.mu_old) {
                mo.x = a.mu_old[(size_t)row * 4];
                mo.y = a.mu_old[(size_t)row * 4 + 1];
                mo.z = a.mu_old[(size_t)row * 4 + 2];
                mo.w = a.mu_old[(size_t)row * 4 + 3];
            }
        }
        const float adv_row = a.adv[row];
        {
            const uint32_t next = tile + nwaves;
            row = row_of(next < ntiles ? next : ntiles - 1u);
            load_obs(row);
        }

        // ---- layer 1
        f4v h1[4], h2[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) h1[t][i] = b1s[16 * t + 4 * g + i];
#pragma unroll
        for (int s = 0; s < N::KS1; ++s) {
            const float b = Z[c * ZS + 4 * s + g];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) h1[nt] = mfma4(W1s[(4 * s + g) * WS + 16 * nt + c], b, h1[nt]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) h1[t][i] = ppo_act<PI>(h1[t][i]);
        // ---- layer 2: k-step (t, i) holds the inputs 16t + 4g + i
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) h2[t][i] = b2s[16 * t + 4 * g + i];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (16 * t + i >= H) continue;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    h2[nt] = mfma4(W2s[(16 * t + 4 * g + i) * WS + 16 * nt + c], h1[t][i], h2[nt]);
            }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) h2[t][i] = ppo_act<PI>(h2[t][i]);
        // ---- layer 3 on the VALU: this lane's 16 neurons, then the four lane groups
        float out[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) out[o] = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int o = 0; o < NO; ++o) out[o] = fmaf(h2[t][i], W3s[(16 * t + 4 * g + i) * 4 + o], out[o]);
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            out[o] += __shfl_xor(out[o], 16);
            out[o] += __shfl_xor(out[o], 32);
            out[o] += b3s[o];
        }

        // ---- head: the row's loss and d loss / d out (not yet divided by m)
        float dout[NO];
        const bool own = valid && g == 0;          // one lane per row writes and counts
        if constexpr (PI) {
            const float ar[4] = {av.x, av.y, av.z, av.w}, mor[4] = {mo.x, mo.y, mo.z, mo.w};
            float A = adv_row;
            if (a.adv_moments) A = (float)(((double)A - adv_mean) / adv_den);
            // the row's scalars in fp64 (a few dozen operations per tile): logp is a sum of terms of
            // size 1..3 whose difference to logp_old is what matters
            double lp = 0.0, kl = 0.0;
            float diff[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                diff[k] = ar[k] - out[k];
                const double zk = ((double)ar[k] - (double)out[k]) * inv_sd[k];
                lp += -0.5 * zk * zk - (double)ls[k] - 0.91893853320467274;      // 0.5 log(2 pi)
            }
            if (a.mu_old) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double dm = (double)mor[k] - (double)out[k];
                    kl += dm * dm * (0.5 * inv_sd[k] * inv_sd[k]);
                }
            }
            const float ratio = (float)exp(lp - (double)lpo);
            const float rc = fminf(fmaxf(ratio, clip_lo), clip_hi);
            const float s1 = ratio * A, s2 = rc * A;
            const bool flows = (ratio >= clip_lo && ratio <= clip_hi) || s1 < s2;
            const float gl = (valid && flows) ? -A * ratio : 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) dout[k] = gl * (diff[k] * inv_var[k]);
            if (own) {
                S[0] += (double)(-fminf(s1, s2));
                S[1] += (double)lpo - lp;
                S[2] += fabsf(ratio - 1.0f) > a.clip ? 1.0 : 0.0;
                S[3] += kl;
                S[4] += (double)ratio;
                if (a.mu_out) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) a.mu_out[(size_t)j * 4 + k] = out[k];
                }
                if (a.logp_out) a.logp_out[j] = (float)lp;
            }
        } else {
            const float dv = out[0] - adv_row;
            dout[0] = valid ? 2.0f * dv : 0.0f;
            if (own) {
                S[0] += (double)dv * (double)dv;
                if (a.logp_out) a.logp_out[j] = out[0];
            }
        }

        if constexpr (GRAD) {
            // ---- layer 3 backward (per lane), dZ2
            f4v dz2[4], dz1[4];
#pragma unroll
            for (int o = 0; o < NO; ++o) b3acc[o] += dout[o];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float dh = 0.0f;
#pragma unroll
                    for (int o = 0; o < NO; ++o) {
                        w3acc[t][i][o] = fmaf(h2[t][i], dout[o], w3acc[t][i][o]);
                        dh = fmaf(dout[o], W3s[(16 * t + 4 * g + i) * 4 + o], dh);
                    }
                    dz2[t][i] = ppo_dact<PI>(h2[t][i], dh);
                    b2acc[t][i] += dz2[t][i];
                }
            // ---- dW2 += H1^T dZ2 over the tile's rows: both through the staging tile [row][neuron]
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ACT[c * AS + 16 * t + 4 * g + i] = h1[t][i];
                    DZ[c * AS + 16 * t + 4 * g + i] = dz2[t][i];
                }
            wave_lds_sync();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float av[4], bv[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    av[t] = ACT[(4 * s + g) * AS + 16 * t + c];
                    bv[t] = DZ[(4 * s + g) * AS + 16 * t + c];
                }
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) acc2[kt][nt] = mfma4(av[kt], bv[nt], acc2[kt][nt]);
            }
            // ---- dH1^T = W2 dZ2^T (A = W2[in][out] read as [in = row of A][out = k]), dZ1
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) dz1[kt] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (16 * t + i >= H) continue;
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
                        dz1[kt] = mfma4(W2s[(16 * kt + c) * WS + 16 * t + 4 * g + i], dz2[t][i], dz1[kt]);
                }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    dz1[t][i] = ppo_dact<PI>(h1[t][i], dz1[t][i]);
                    b1acc[t][i] += dz1[t][i];
                }
            // ---- dW1 += Z^T dZ1
            wave_lds_sync();                       // every lane has read dZ2 from the staging tile
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) DZ[c * AS + 16 * t + 4 * g + i] = dz1[t][i];
            wave_lds_sync();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float av[N::KT1], bv[4];
#pragma unroll
                for (int kt = 0; kt < N::KT1; ++kt) av[kt] = Z[(4 * s + g) * ZS + 16 * kt + c];
#pragma unroll
                for (int t = 0; t < 4; ++t) bv[t] = DZ[(4 * s + g) * AS + 16 * t + c];
#pragma unroll
                for (int kt = 0; kt < N::KT1; ++kt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) acc1[kt][nt] = mfma4(av[kt], bv[nt], acc1[kt][nt]);
            }
        }
        wave_lds_sync();                           // the next tile overwrites Z and the staging tile
    }

    // ---- the block's summary: lanes, then waves, in a fixed order
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double v = S[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
        if (lane == 0) sred[wave][k] = v;
    }
    __syncthreads();                               // also: every wave is done with the weights in LDS
    if (tid < PPO_SUM) {
        double v = 0.0;
        if (tid >= 1 && tid <= 5)
            for (int w = 0; w < PPO_WAVES; ++w) v += sred[w][tid - 1];
        a.part_sum[(size_t)ppo_block_of(ka) * PPO_SUM + tid] = v;
    }

    if constexpr (GRAD) {
        // ---- the block's gradient: the waves add into LDS in wave order (wave 0 stores)
        float* red = lds;
        float db3[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) db3[o] = sum_rows(b3acc[o]);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                b1acc[t][i] = sum_rows(b1acc[t][i]);
                b2acc[t][i] = sum_rows(b2acc[t][i]);
#pragma unroll
                for (int o = 0; o < NO; ++o) w3acc[t][i][o] = sum_rows(w3acc[t][i][o]);
            }
        for (int w = 0; w < PPO_WAVES; ++w) {
            if (wave == w) {
                const bool first = w == 0;
                auto put = [&](int p, float v) { red[p] = first ? v : red[p] + v; };
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const int n = 16 * nt + c;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
#pragma unroll
                        for (int kt = 0; kt < N::KT1; ++kt) {
                            const int k = 16 * kt + 4 * g + i;
                            if (k < D && n < H) put(N::W1 + k * H + n, acc1[kt][nt][i]);
                        }
#pragma unroll
                        for (int kt = 0; kt < 4; ++kt) {
                            const int k = 16 * kt + 4 * g + i;
                            if (k < H && n < H) put(N::W2 + k * H + n, acc2[kt][nt][i]);
                        }
                    }
                }
                if (c == 0) {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int k = 16 * t + 4 * g + i;
                            if (k < H) {
                                put(N::B1 + k, b1acc[t][i]);
                                put(N::B2 + k, b2acc[t][i]);
#pragma unroll
                                for (int o = 0; o < NO; ++o) put(N::W3 + k * NO + o, w3acc[t][i][o]);
                            }
                        }
                    if (g == 0) {
#pragma unroll
                        for (int o = 0; o < NO; ++o) put(N::B3 + o, db3[o]);
                    }
                }
            }
            __syncthreads();
        }
        float* dst = a.part_grad + (size_t)ppo_block_of(ka) * N::NPAR;
        for (int p = tid; p < N::NPAR; p += PPO_BLOCK) dst[p] = red[p];
    }
}

// Block partials -> gradient slice and summary: fp64 sums in block-index order, divided by m, one
// rounding to fp32.  grad == nullptr: the summary only.  gate: as PpoArgs::gate.
__global__ void __launch_bounds__(256) ppo_merge_kernel(const float* __restrict__ part_grad,
                                                        const double* __restrict__ part_sum, uint32_t blocks,
                                                        uint32_t npar, uint32_t m, float* __restrict__ grad,
                                                        double* __restrict__ summary,
                                                        const uint32_t* __restrict__ gate) {
    if (gate && *gate != 0u) return;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (grad && p < npar) {
        double acc = 0.0;
#pragma unroll 8
        for (uint32_t b = 0; b < blocks; ++b) acc += (double)part_grad[(size_t)b * npar + p];
        grad[p] = (float)(acc / (double)m);
    }
    if (blockIdx.x == 0 && threadIdx.x < PPO_SUM) {
        const uint32_t k = threadIdx.x;
        double acc = 0.0;
        for (uint32_t b = 0; b < blocks; ++b) acc += part_sum[(size_t)b * PPO_SUM + k];
        summary[k] = k == 0 ? (double)m : acc / (double)m;      // slots 6, 7 (and the unused ones) sum zeros
    }
}

// ppo_merge_kernel for P members: blocks [k mblocks, (k + 1) mblocks) are member k's merge launch on
// member k's slice of the scratch (scratch_stride bytes apart), the same sums in the same order and
// the same single rounding, written to grad + k grad_stride (already offset to the network's slice)
// and summary + 8 k.  gate: member k's word is gate[4 k].
__global__ void __launch_bounds__(256) ppo_merge_pop_kernel(const float* __restrict__ part_grad,
                                                            const double* __restrict__ part_sum, size_t scratch_stride,
                                                            uint32_t mblocks, uint32_t blocks, uint32_t npar, uint32_t m,
                                                            float* __restrict__ grad, size_t grad_stride,
                                                            double* __restrict__ summary,
                                                            const uint32_t* __restrict__ gate) {
    const uint32_t k = blockIdx.x / mblocks, bx = blockIdx.x - k * mblocks;
    if (gate && gate[4u * (size_t)k] != 0u) return;
    part_grad = reinterpret_cast<const float*>(reinterpret_cast<const char*>(part_grad) + k * scratch_stride);
    part_sum = reinterpret_cast<const double*>(reinterpret_cast<const char*>(part_sum) + k * scratch_stride);
    const uint32_t p = bx * 256u + threadIdx.x;
    if (grad && p < npar) {
        double acc = 0.0;
#pragma unroll 8
        for (uint32_t b = 0; b < blocks; ++b) acc += (double)part_grad[(size_t)b * npar + p];
        grad[k * grad_stride + p] = (float)(acc / (double)m);
    }
    if (bx == 0 && threadIdx.x < PPO_SUM) {
        const uint32_t j = threadIdx.x;
        double acc = 0.0;
        for (uint32_t b = 0; b < blocks; ++b) acc += part_sum[(size_t)b * PPO_SUM + j];
        summary[(size_t)PPO_SUM * k + j] = j == 0 ? (double)m : acc / (double)m;
    }
}

// Block partials -> one rank-partial block of doubles (data-parallel updates; cf2_ppo_reduce of
// cf2sim_reduce.hip is the second level): out[0] = m, out[1..7] = the fp64 sums of the summary slots,
// out[8 + p] = the fp64 sum of gradient word p, all in block-index order as ppo_merge_kernel sums
// them, not divided and not rounded.  with_grad == 0, and the words past npar up to `words` (the
// block's fixed size less the head): 0.  blocks == 0 (m == 0): a zeroed block.  gate: as PpoArgs::gate.
__global__ void __launch_bounds__(256) ppo_partial_merge_kernel(const float* __restrict__ part_grad,
                                                                const double* __restrict__ part_sum, uint32_t blocks,
                                                                uint32_t npar, uint32_t words, uint32_t m, int with_grad,
                                                                double* __restrict__ out,
                                                                const uint32_t* __restrict__ gate) {
    if (gate && *gate != 0u) return;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < words) {
        double acc = 0.0;
        if (with_grad && p < npar) {
#pragma unroll 8
            for (uint32_t b = 0; b < blocks; ++b) acc += (double)part_grad[(size_t)b * npar + p];
        }
        out[PPO_SUM + p] = acc;
    }
    if (blockIdx.x == 0 && threadIdx.x < PPO_SUM) {
        const uint32_t k = threadIdx.x;
        double acc = 0.0;
        for (uint32_t b = 0; b < blocks; ++b) acc += part_sum[(size_t)b * PPO_SUM + k];
        out[k] = k == 0 ? (double)m : acc;
    }
}

// {mean, M2} taken over *count rows -> {mean, M2 rows / *count}: ppo_kernel divides M2 by its row
// count `rows` (PpoArgs::n), so it standardises with sqrt(M2 / *count), the deviation of all ranks'
// rows.  *count == rows: the factor is exactly 1 and the moments pass through bit for bit.
__global__ void ppo_moments_rescale_kernel(const double* __restrict__ mom, double rows, const double* __restrict__ count,
                                           double* __restrict__ out, const uint32_t* __restrict__ gate) {
    if (gate && *gate != 0u) return;
    out[0] = mom[0];
    out[1] = mom[1] * (rows / *count);
}

static uint32_t ppo_blocks(uint32_t m) {
    const uint32_t tiles = (m + 15u) / 16u, want = (tiles + PPO_WAVES - 1) / PPO_WAVES;
    return want < PPO_MAX_BLOCKS ? want : PPO_MAX_BLOCKS;
}
static uint32_t ppo_npar_max(uint32_t D) { return D == 34 ? PpoNet<34, false>::NPAR : PpoNet<42, false>::NPAR; }

template <int D, bool PI>
static int ppo_launch(PpoArgs a, float* grad, double* summary, void* scratch, hipStream_t s) {
    using N = PpoNet<D, PI>;
    const uint32_t blocks = ppo_blocks(a.m);
    a.part_sum = static_cast<double*>(scratch);
    a.part_grad = reinterpret_cast<float*>(a.part_sum + (size_t)PPO_MAX_BLOCKS * PPO_SUM);
    if (grad)
        hipLaunchKernelGGL((ppo_kernel<D, PI, true>), dim3(blocks), dim3(PPO_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL((ppo_kernel<D, PI, false>), dim3(blocks), dim3(PPO_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    const uint32_t mblocks = grad ? (N::NPAR + 255u) / 256u : 1u;
    hipLaunchKernelGGL(ppo_merge_kernel, dim3(mblocks), dim3(256), 0, s, a.part_grad, a.part_sum, blocks,
                       (uint32_t)N::NPAR, a.m, grad ? grad + N::BASE : nullptr, summary, a.gate);
    e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}

static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

// a member's slice of the population scratch: the stand-alone scratch, rounded up to 16 bytes
static size_t ppo_pop_slice_bytes(uint32_t m, uint32_t D) {
    const size_t one = (size_t)PPO_MAX_BLOCKS * PPO_SUM * sizeof(double) + (size_t)ppo_blocks(m) * ppo_npar_max(D) * sizeof(float);
    return (one + 15u) & ~(size_t)15u;
}

// the two launches of a population call; p.base, the strides and p.clip are filled in by the caller
template <int D, bool PI>
static int ppo_pop_launch(PpoPopArgs p, uint32_t members, float* grad, double* summary, void* scratch, hipStream_t s) {
    using N = PpoNet<D, PI>;
    p.bpm = ppo_blocks(p.base.m);
    p.s_scratch = ppo_pop_slice_bytes(p.base.m, D);
    p.base.part_sum = static_cast<double*>(scratch);
    p.base.part_grad = reinterpret_cast<float*>(p.base.part_sum + (size_t)PPO_MAX_BLOCKS * PPO_SUM);
    const uint32_t grid = members * p.bpm;         // below 2^31: checked by the caller
    if (grad)
        hipLaunchKernelGGL((ppo_kernel<D, PI, true, true>), dim3(grid), dim3(PPO_BLOCK), 0, s, p);
    else
        hipLaunchKernelGGL((ppo_kernel<D, PI, false, true>), dim3(grid), dim3(PPO_BLOCK), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    const uint32_t mblocks = grad ? (N::NPAR + 255u) / 256u : 1u;
    hipLaunchKernelGGL(ppo_merge_pop_kernel, dim3(members * mblocks), dim3(256), 0, s, p.base.part_grad, p.base.part_sum,
                       p.s_scratch, mblocks, p.bpm, (uint32_t)N::NPAR, p.base.m, grad ? grad + N::BASE : nullptr, p.s_w,
                       summary, p.base.gate);
    e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}

// a grid of members * blocks per member that the launch cannot take
static bool ppo_pop_grid_overflows(uint32_t members, uint32_t m, uint32_t D) {
    const uint32_t merge = (ppo_npar_max(D) + 255u) / 256u, grad = ppo_blocks(m);      // blocks per member, either launch
    return (uint64_t)members * (grad > merge ? grad : merge) >= (1ull << 31);
}

// the fixed size of a rank-partial block: the head and the larger (value) slice
template <int D>
constexpr uint32_t ppo_partial_doubles() { return PPO_SUM + PpoNet<D, false>::NPAR; }
static_assert(PpoNet<34, false>::NPAR >= PpoNet<34, true>::NPAR + 6 && PpoNet<42, false>::NPAR >= PpoNet<42, true>::NPAR + 6,
              "the policy call's rescaled moments fit behind its block partials in the scratch");

// the second launch of the rank-partial calls (m == 0: the only one, a zeroed block)
template <int D, bool PI>
static int partial_merge_launch(const float* part_grad, const double* part_sum, uint32_t blocks, uint32_t m,
                                bool with_grad, double* out, const uint32_t* gate, hipStream_t s) {
    constexpr uint32_t words = ppo_partial_doubles<D>() - PPO_SUM;
    hipLaunchKernelGGL(ppo_partial_merge_kernel, dim3((words + 255u) / 256u), dim3(256), 0, s, part_grad, part_sum, blocks,
                       (uint32_t)PpoNet<D, PI>::NPAR, words, m, with_grad ? 1 : 0, out, gate);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}

// count: the device word holding the rows adv_moments was taken over (policy with adv_moments only)
template <int D, bool PI>
static int ppo_partial_launch(PpoArgs a, bool with_grad, const double* count, double* out, void* scratch,
                              hipStream_t s) {
    using N = PpoNet<D, PI>;
    const uint32_t blocks = ppo_blocks(a.m);
    a.part_sum = static_cast<double*>(scratch);
    a.part_grad = reinterpret_cast<float*>(a.part_sum + (size_t)PPO_MAX_BLOCKS * PPO_SUM);
    if (blocks == 0) return partial_merge_launch<D, PI>(nullptr, nullptr, 0, 0, false, out, a.gate, s);
    if (PI && a.adv_moments) {
        // behind the block partials, 8-byte aligned: the scratch is sized for the value slice
        double* mom = reinterpret_cast<double*>(a.part_grad + (((size_t)blocks * N::NPAR + 1u) & ~(size_t)1u));
        hipLaunchKernelGGL(ppo_moments_rescale_kernel, dim3(1), dim3(1), 0, s, a.adv_moments, (double)a.n, count, mom,
                           a.gate);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e);
        a.adv_moments = mom;
    }
    if (with_grad)
        hipLaunchKernelGGL((ppo_kernel<D, PI, true>), dim3(blocks), dim3(PPO_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL((ppo_kernel<D, PI, false>), dim3(blocks), dim3(PPO_BLOCK), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    return partial_merge_launch<D, PI>(a.part_grad, a.part_sum, blocks, a.m, with_grad, out, a.gate, s);
}

// ---------------------------------------------------------------------------------------------
// Fisher-vector product of the policy (the natural-gradient updates, cf2sim_natgrad.hip).  For a
// Gaussian policy whose log_std is not trained the KL to the old policy is
// sum_k (mu_old_k - mu_k)^2 / (2 sigma_k^2); its Hessian at mu = mu_old is the Gauss-Newton matrix
// F = (1/m) sum_rows J^T Sigma^-1 J exactly (the term with the net's second derivatives is multiplied
// by mu - mu_old = 0).  F v per 16-row tile: the primal forward of ppo_kernel up to h2, a tangent
// pass with the weights' direction v = (V1 vb1 V2 vb2 V3 vb3) riding on the same B operands,
//     th1 = relu'(z1) (V1^T z + vb1)
//     th2 = relu'(z2) (V2^T h1 + W2^T th1 + vb2)
//     tmu = V3^T h2 + W3^T th2 + vb3                           (= J v, on the VALU like layer 3)
// then dout = tmu / sigma^2 through the backward pass and the gradient GEMMs of ppo_kernel.  The
// tangents are dead once tmu is known, so the accumulators, the block reduction and ppo_merge_kernel
// are the gradient kernel's; the direction needs a second zero-padded LDS copy (the map of the
// weights, moved behind the waves' staging tiles).  summary[1] = v^T F v = mean_rows sum_k tmu_k^2 /
// sigma_k^2, in fp64.
// ---------------------------------------------------------------------------------------------
struct FisherArgs {
    const float* W;
    const float* V;              // the direction: a whole flat block, the words [P_W1, P_LOGSTD) are read
    const float* obs;
    const uint32_t* idx;
    double* part_sum;            // [blocks][PPO_SUM]
    float* part_grad;            // [blocks][NPAR]
    uint32_t n, m;
    const uint32_t* gate;        // as PpoArgs::gate
};

// P members in one launch (cf2_ppo_fisher_vec_pop; ppo_fisher_kernel<D, true>), as PpoPopArgs: `base`
// holds member 0's pointers, member k's lie k strides (in elements) further on; block b serves member
// b / bpm as that member's block b % bpm through the one kernel body.  s_idx == 0: one index list
// that every member reads.  The gate word of member k is gate[4 k].
struct FisherPopArgs {
    FisherArgs base;             // n, m shared; part_sum, part_grad: member 0's slice of the scratch
    size_t s_w, s_v, s_obs, s_idx;
    size_t s_scratch;            // bytes between the members' scratch slices
    uint32_t bpm;
};

__device__ __forceinline__ FisherArgs fisher_member_args(const FisherPopArgs& p, const uint32_t k) {
    FisherArgs a = p.base;
    a.W += k * p.s_w;
    a.V += k * p.s_v;
    a.obs += k * p.s_obs;
    if (a.idx) a.idx += k * p.s_idx;
    a.part_sum = reinterpret_cast<double*>(reinterpret_cast<char*>(a.part_sum) + k * p.s_scratch);
    a.part_grad = reinterpret_cast<float*>(reinterpret_cast<char*>(a.part_grad) + k * p.s_scratch);
    if (a.gate) a.gate += 4u * (size_t)k;
    return a;
}

// the kernel argument and block geometry of an instance, as PpoKernelArgs above (the reason is there)
template <bool POP> struct FisherKernelArgs { using type = FisherArgs; };
template <> struct FisherKernelArgs<true> { using type = FisherPopArgs; };
__device__ __forceinline__ const FisherArgs& fisher_args_of(const FisherArgs& a) { return a; }
__device__ __forceinline__ FisherArgs fisher_args_of(const FisherPopArgs& p) {
    return fisher_member_args(p, blockIdx.x / p.bpm);
}
__device__ __forceinline__ uint32_t ppo_block_of(const FisherArgs&) { return blockIdx.x; }
__device__ __forceinline__ uint32_t ppo_block_of(const FisherPopArgs& p) { return blockIdx.x % p.bpm; }
__device__ __forceinline__ uint32_t ppo_nblocks_of(const FisherArgs&) { return gridDim.x; }
__device__ __forceinline__ uint32_t ppo_nblocks_of(const FisherPopArgs& p) { return p.bpm; }

template <int D, bool POP = false>
__global__ void __launch_bounds__(PPO_BLOCK) ppo_fisher_kernel(const typename FisherKernelArgs<POP>::type ka) {
    using N = PpoNet<D, true>;
    using L = PolicyLayout<D>;
    const FisherArgs& a = fisher_args_of(ka);
    constexpr int H = N::H, NO = N::NO, WS = PPO_WS, AS = PPO_AS, ZS = PPO_ZS;
    constexpr int TAN = N::LDS_FLOATS;             // the direction's copy: the map of the weights, shifted
    constexpr int TAN_FLOATS = N::S_MEAN;          // W1 W2 W3 b1 b2 b3
    if (a.gate && *a.gate != 0u) return;
    __shared__ __attribute__((aligned(16))) float lds[N::LDS_FLOATS + TAN_FLOATS];
    __shared__ double sred[PPO_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    float* W1s = lds + N::S_W1;
    float* W2s = lds + N::S_W2;
    float* W3s = lds + N::S_W3;
    float* b1s = lds + N::S_B1;
    float* b2s = lds + N::S_B2;
    float* V1s = lds + TAN + N::S_W1;
    float* V2s = lds + TAN + N::S_W2;
    float* V3s = lds + TAN + N::S_W3;
    float* vb1s = lds + TAN + N::S_B1;
    float* vb2s = lds + TAN + N::S_B2;
    float* vb3s = lds + TAN + N::S_B3;
    float* means = lds + N::S_MEAN;
    float* scales = lds + N::S_SCALE;
    float* Z = lds + N::S_WAVE + wave * N::WAVE_FLOATS + N::WAVE_Z;
    float* ACT = lds + N::S_WAVE + wave * N::WAVE_FLOATS + N::WAVE_ACT;
    float* DZ = lds + N::S_WAVE + wave * N::WAVE_FLOATS + N::WAVE_DZ;

    // ---- the net's weights and the direction, zero-padded to 64 neurons per layer
    const float* Wn = a.W + N::BASE;
    const float* Vn = a.V + N::BASE;
    for (int e = tid; e < N::KP1 * 64; e += PPO_BLOCK) {
        const int k = e >> 6, n = e & 63;
        const bool in = k < D && n < H;
        W1s[k * WS + n] = in ? Wn[N::W1 + k * H + n] : 0.0f;
        V1s[k * WS + n] = in ? Vn[N::W1 + k * H + n] : 0.0f;
    }
    for (int e = tid; e < 64 * 64; e += PPO_BLOCK) {
        const int k = e >> 6, n = e & 63;
        const bool in = k < H && n < H;
        W2s[k * WS + n] = in ? Wn[N::W2 + k * H + n] : 0.0f;
        V2s[k * WS + n] = in ? Vn[N::W2 + k * H + n] : 0.0f;
    }
    {
        const int k = tid >> 2, o = tid & 3;
        const bool in = k < H && o < NO;
        W3s[tid] = in ? Wn[N::W3 + k * NO + o] : 0.0f;
        V3s[tid] = in ? Vn[N::W3 + k * NO + o] : 0.0f;
    }
    if (tid < 64) {
        b1s[tid] = tid < H ? Wn[N::B1 + tid] : 0.0f;
        b2s[tid] = tid < H ? Wn[N::B2 + tid] : 0.0f;
        vb1s[tid] = tid < H ? Vn[N::B1 + tid] : 0.0f;
        vb2s[tid] = tid < H ? Vn[N::B2 + tid] : 0.0f;
        if (tid < 4) vb3s[tid] = tid < NO ? Vn[N::B3 + tid] : 0.0f;
        if (tid < 48) {
            means[tid] = tid < D ? a.W[L::O_MEAN + tid] : 0.0f;
            scales[tid] = tid < D ? a.W[L::O_SCALE + tid] : 0.0f;
        }
    }
    for (int e = lane; e < 16 * ZS; e += 64) Z[e] = 0.0f;        // the columns past D stay 0
    __syncthreads();

    // ---- per-lane constants
    float inv_var[4];
    double inv_var64[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        inv_var64[k] = exp(-2.0 * (double)a.W[L::P_LOGSTD + k]);
        inv_var[k] = (float)inv_var64[k];
    }

    // ---- accumulators
    f4v acc1[N::KT1][4], acc2[4][4];
    float w3acc[4][4][NO], b1acc[4][4], b2acc[4][4], b3acc[NO];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int kt = 0; kt < N::KT1; ++kt) acc1[kt][t] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) acc2[kt][t] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            b1acc[t][i] = 0.0f;
            b2acc[t][i] = 0.0f;
#pragma unroll
            for (int o = 0; o < NO; ++o) w3acc[t][i][o] = 0.0f;
        }
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) b3acc[o] = 0.0f;
    double S = 0.0;

    const uint32_t ntiles = (a.m + 15u) / 16u, nwaves = ppo_nblocks_of(ka) * PPO_WAVES;
    // the row of position 16 tile + c; a position past m reads row m - 1 and contributes nothing
    auto row_of = [&](uint32_t tile) {
        const uint32_t jc = __builtin_elementwise_min(tile * 16u + (uint32_t)c, a.m - 1u);
        return a.idx ? __builtin_elementwise_min(a.idx[jc], a.n - 1u) : jc;
    };
    constexpr int ZIT = (16 * D + 63) / 64;
    float xr[ZIT];
    auto load_obs = [&](uint32_t row) {
#pragma unroll
        for (int it = 0; it < ZIT; ++it) {
            const int e = it * 64 + lane, ee = e < 16 * D ? e : 16 * D - 1;
            const int r = ee / D, k = ee - r * D;
            xr[it] = a.obs[(size_t)__shfl(row, r) * D + k];
        }
    };
    uint32_t tile = ppo_block_of(ka) * PPO_WAVES + wave;
    uint32_t row = row_of(tile < ntiles ? tile : ntiles - 1u);
    load_obs(row);
    for (; tile < ntiles; tile += nwaves) {
        const uint32_t j = tile * 16u + (uint32_t)c;
        const bool valid = j < a.m;
#pragma unroll
        for (int it = 0; it < ZIT; ++it) {
            const int e = it * 64 + lane, ee = e < 16 * D ? e : 16 * D - 1;
            const int r = ee / D, k = ee - r * D;
            if (e < 16 * D) Z[r * ZS + k] = (xr[it] - means[k]) * scales[k];
        }
        wave_lds_sync();
        {
            const uint32_t next = tile + nwaves;
            row = row_of(next < ntiles ? next : ntiles - 1u);
            load_obs(row);
        }

        // ---- layer 1 and its tangent: the same B operand
        f4v h1[4], h2[4], t1[4], t2[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                h1[t][i] = b1s[16 * t + 4 * g + i];
                t1[t][i] = vb1s[16 * t + 4 * g + i];
            }
#pragma unroll
        for (int s = 0; s < N::KS1; ++s) {
            const float b = Z[c * ZS + 4 * s + g];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                h1[nt] = mfma4(W1s[(4 * s + g) * WS + 16 * nt + c], b, h1[nt]);
                t1[nt] = mfma4(V1s[(4 * s + g) * WS + 16 * nt + c], b, t1[nt]);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                h1[t][i] = relu(h1[t][i]);
                t1[t][i] = ppo_dact<true>(h1[t][i], t1[t][i]);
            }
        // ---- layer 2: k-step (t, i) holds the inputs 16t + 4g + i
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                h2[t][i] = b2s[16 * t + 4 * g + i];
                t2[t][i] = vb2s[16 * t + 4 * g + i];
            }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (16 * t + i >= H) continue;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const float w = W2s[(16 * t + 4 * g + i) * WS + 16 * nt + c];
                    h2[nt] = mfma4(w, h1[t][i], h2[nt]);
                    t2[nt] = mfma4(V2s[(16 * t + 4 * g + i) * WS + 16 * nt + c], h1[t][i], t2[nt]);
                    t2[nt] = mfma4(w, t1[t][i], t2[nt]);
                }
            }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                h2[t][i] = relu(h2[t][i]);
                t2[t][i] = ppo_dact<true>(h2[t][i], t2[t][i]);
            }
        // ---- J v on the VALU: this lane's 16 neurons, then the four lane groups
        float tmu[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) tmu[o] = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int o = 0; o < NO; ++o) {
                    tmu[o] = fmaf(h2[t][i], V3s[(16 * t + 4 * g + i) * 4 + o], tmu[o]);
                    tmu[o] = fmaf(t2[t][i], W3s[(16 * t + 4 * g + i) * 4 + o], tmu[o]);
                }
        float dout[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            tmu[o] += __shfl_xor(tmu[o], 16);
            tmu[o] += __shfl_xor(tmu[o], 32);
            tmu[o] += vb3s[o];
            dout[o] = valid ? tmu[o] * inv_var[o] : 0.0f;
        }
        if (valid && g == 0) {                     // one lane per row counts
#pragma unroll
            for (int o = 0; o < NO; ++o) S += (double)tmu[o] * (double)tmu[o] * inv_var64[o];
        }

        // ---- layer 3 backward (per lane), dZ2
        f4v dz2[4], dz1[4];
#pragma unroll
        for (int o = 0; o < NO; ++o) b3acc[o] += dout[o];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float dh = 0.0f;
#pragma unroll
                for (int o = 0; o < NO; ++o) {
                    w3acc[t][i][o] = fmaf(h2[t][i], dout[o], w3acc[t][i][o]);
                    dh = fmaf(dout[o], W3s[(16 * t + 4 * g + i) * 4 + o], dh);
                }
                dz2[t][i] = ppo_dact<true>(h2[t][i], dh);
                b2acc[t][i] += dz2[t][i];
            }
        // ---- dW2 += H1^T dZ2 over the tile's rows: both through the staging tile [row][neuron]
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ACT[c * AS + 16 * t + 4 * g + i] = h1[t][i];
                DZ[c * AS + 16 * t + 4 * g + i] = dz2[t][i];
            }
        wave_lds_sync();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                av[t] = ACT[(4 * s + g) * AS + 16 * t + c];
                bv[t] = DZ[(4 * s + g) * AS + 16 * t + c];
            }
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc2[kt][nt] = mfma4(av[kt], bv[nt], acc2[kt][nt]);
        }
        // ---- dH1^T = W2 dZ2^T, dZ1
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) dz1[kt] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (16 * t + i >= H) continue;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
                    dz1[kt] = mfma4(W2s[(16 * kt + c) * WS + 16 * t + 4 * g + i], dz2[t][i], dz1[kt]);
            }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dz1[t][i] = ppo_dact<true>(h1[t][i], dz1[t][i]);
                b1acc[t][i] += dz1[t][i];
            }
        // ---- dW1 += Z^T dZ1
        wave_lds_sync();                           // every lane has read dZ2 from the staging tile
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) DZ[c * AS + 16 * t + 4 * g + i] = dz1[t][i];
        wave_lds_sync();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float av[N::KT1], bv[4];
#pragma unroll
            for (int kt = 0; kt < N::KT1; ++kt) av[kt] = Z[(4 * s + g) * ZS + 16 * kt + c];
#pragma unroll
            for (int t = 0; t < 4; ++t) bv[t] = DZ[(4 * s + g) * AS + 16 * t + c];
#pragma unroll
            for (int kt = 0; kt < N::KT1; ++kt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc1[kt][nt] = mfma4(av[kt], bv[nt], acc1[kt][nt]);
        }
        wave_lds_sync();                           // the next tile overwrites Z and the staging tile
    }

    // ---- the block's summary: lanes, then waves, in a fixed order
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) S += __shfl_xor(S, d);
    if (lane == 0) sred[wave] = S;
    __syncthreads();                               // also: every wave is done with the weights in LDS
    if (tid < PPO_SUM) {
        double v = 0.0;
        if (tid == 1)
            for (int w = 0; w < PPO_WAVES; ++w) v += sred[w];
        a.part_sum[(size_t)ppo_block_of(ka) * PPO_SUM + tid] = v;
    }

    // ---- the block's product: the waves add into LDS in wave order (wave 0 stores)
    float* red = lds;
    float db3[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) db3[o] = sum_rows(b3acc[o]);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            b1acc[t][i] = sum_rows(b1acc[t][i]);
            b2acc[t][i] = sum_rows(b2acc[t][i]);
#pragma unroll
            for (int o = 0; o < NO; ++o) w3acc[t][i][o] = sum_rows(w3acc[t][i][o]);
        }
    for (int w = 0; w < PPO_WAVES; ++w) {
        if (wave == w) {
            const bool first = w == 0;
            auto put = [&](int p, float v) { red[p] = first ? v : red[p] + v; };
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + c;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int kt = 0; kt < N::KT1; ++kt) {
                        const int k = 16 * kt + 4 * g + i;
                        if (k < D && n < H) put(N::W1 + k * H + n, acc1[kt][nt][i]);
                    }
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt) {
                        const int k = 16 * kt + 4 * g + i;
                        if (k < H && n < H) put(N::W2 + k * H + n, acc2[kt][nt][i]);
                    }
                }
            }
            if (c == 0) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int k = 16 * t + 4 * g + i;
                        if (k < H) {
                            put(N::B1 + k, b1acc[t][i]);
                            put(N::B2 + k, b2acc[t][i]);
#pragma unroll
                            for (int o = 0; o < NO; ++o) put(N::W3 + k * NO + o, w3acc[t][i][o]);
                        }
                    }
                if (g == 0) {
#pragma unroll
                    for (int o = 0; o < NO; ++o) put(N::B3 + o, db3[o]);
                }
            }
        }
        __syncthreads();
    }
    float* dst = a.part_grad + (size_t)ppo_block_of(ka) * N::NPAR;
    for (int p = tid; p < N::NPAR; p += PPO_BLOCK) dst[p] = red[p];
}

template <int D>
static int fisher_launch(FisherArgs a, float* out, double* summary, void* scratch, hipStream_t s) {
    using N = PpoNet<D, true>;
    const uint32_t blocks = ppo_blocks(a.m);
    a.part_sum = static_cast<double*>(scratch);
    a.part_grad = reinterpret_cast<float*>(a.part_sum + (size_t)PPO_MAX_BLOCKS * PPO_SUM);
    hipLaunchKernelGGL((ppo_fisher_kernel<D>), dim3(blocks), dim3(PPO_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(ppo_merge_kernel, dim3((N::NPAR + 255u) / 256u), dim3(256), 0, s, a.part_grad, a.part_sum, blocks,
                       (uint32_t)N::NPAR, a.m, out + N::BASE, summary, a.gate);
    e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}

// the two launches of cf2_ppo_fisher_vec_pop; p.base and the strides are filled in by the caller
template <int D>
static int fisher_pop_launch(FisherPopArgs p, uint32_t members, float* out, size_t out_stride, double* summary,
                             void* scratch, hipStream_t s) {
    using N = PpoNet<D, true>;
    p.bpm = ppo_blocks(p.base.m);
    p.s_scratch = ppo_pop_slice_bytes(p.base.m, D);
    p.base.part_sum = static_cast<double*>(scratch);
    p.base.part_grad = reinterpret_cast<float*>(p.base.part_sum + (size_t)PPO_MAX_BLOCKS * PPO_SUM);
    const uint32_t grid = members * p.bpm;         // below 2^31: checked by the caller
    hipLaunchKernelGGL((ppo_fisher_kernel<D, true>), dim3(grid), dim3(PPO_BLOCK), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    const uint32_t mblocks = (N::NPAR + 255u) / 256u;
    hipLaunchKernelGGL(ppo_merge_pop_kernel, dim3(members * mblocks), dim3(256), 0, s, p.base.part_grad, p.base.part_sum,
                       p.s_scratch, mblocks, p.bpm, (uint32_t)N::NPAR, p.base.m, out + N::BASE, out_stride, summary,
                       p.base.gate);
    e = hipGetLastError();
    return e == hipSuccess ? CF2_OK : hip_fail(e);
}

template <int D>
static int fisher_partial_launch(FisherArgs a, double* out, void* scratch, hipStream_t s) {
    const uint32_t blocks = ppo_blocks(a.m);
    a.part_sum = static_cast<double*>(scratch);
    a.part_grad = reinterpret_cast<float*>(a.part_sum + (size_t)PPO_MAX_BLOCKS * PPO_SUM);
    if (blocks == 0) return partial_merge_launch<D, true>(nullptr, nullptr, 0, 0, false, out, a.gate, s);
    hipLaunchKernelGGL((ppo_fisher_kernel<D>), dim3(blocks), dim3(PPO_BLOCK), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    return partial_merge_launch<D, true>(a.part_grad, a.part_sum, blocks, a.m, true, out, a.gate, s);
}

}  // namespace cf2

using namespace cf2;

extern "C" size_t cf2_ppo_scratch_bytes(uint32_t m, uint32_t obs_dim) {
    if (obs_dim != 34 && obs_dim != 42) return 0;
    return (size_t)PPO_MAX_BLOCKS * PPO_SUM * sizeof(double) + (size_t)ppo_blocks(m) * ppo_npar_max(obs_dim) * sizeof(float);
}

static int policy_grad(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, const float* act_dev,
                       const float* logp_old_dev, const float* adv_dev, uint32_t n, const uint32_t* idx_dev, uint32_t m,
                       const double* adv_moments_dev, float clip_ratio, const float* mu_old_dev, float* mu_out_dev,
                       float* logp_out_dev, float* grad_dev, double* summary_dev, void* scratch_dev,
                       const uint32_t* ctrl_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (m == 0) return CF2_OK;
    if (!weights_dev || !obs_dev || !act_dev || !logp_old_dev || !adv_dev || !summary_dev || !scratch_dev || n == 0 ||
        (!idx_dev && m > n))
        return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(obs_dev, 8) || misaligned(act_dev, 16) || misaligned(logp_old_dev, 4) ||
        misaligned(adv_dev, 4) || misaligned(idx_dev, 4) || misaligned(adv_moments_dev, 8) || misaligned(mu_old_dev, 4) ||
        misaligned(mu_out_dev, 4) || misaligned(logp_out_dev, 4) || misaligned(grad_dev, 4) || misaligned(summary_dev, 8) ||
        misaligned(scratch_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    PpoArgs a = {weights_dev, obs_dev, act_dev, logp_old_dev, adv_dev, idx_dev, adv_moments_dev, mu_old_dev, mu_out_dev,
                 logp_out_dev, nullptr, nullptr, n, m, clip_ratio, ctrl_dev};
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? ppo_launch<34, true>(a, grad_dev, summary_dev, scratch_dev, s)
                         : ppo_launch<42, true>(a, grad_dev, summary_dev, scratch_dev, s);
}

extern "C" int cf2_ppo_policy_grad(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, const float* act_dev,
                                   const float* logp_old_dev, const float* adv_dev, uint32_t n, const uint32_t* idx_dev,
                                   uint32_t m, const double* adv_moments_dev, float clip_ratio, const float* mu_old_dev,
                                   float* mu_out_dev, float* logp_out_dev, float* grad_dev, double* summary_dev,
                                   void* scratch_dev, void* stream) {
    return policy_grad(weights_dev, obs_dim, obs_dev, act_dev, logp_old_dev, adv_dev, n, idx_dev, m, adv_moments_dev,
                       clip_ratio, mu_old_dev, mu_out_dev, logp_out_dev, grad_dev, summary_dev, scratch_dev, nullptr,
                       stream);
}

extern "C" int cf2_ppo_policy_grad_gated(const float* weights_dev, uint32_t obs_dim, const float* obs_dev,
                                         const float* act_dev, const float* logp_old_dev, const float* adv_dev, uint32_t n,
                                         const uint32_t* idx_dev, uint32_t m, const double* adv_moments_dev,
                                         float clip_ratio, const float* mu_old_dev, float* mu_out_dev, float* logp_out_dev,
                                         float* grad_dev, double* summary_dev, void* scratch_dev,
                                         const uint32_t* ctrl_dev, void* stream) {
    return policy_grad(weights_dev, obs_dim, obs_dev, act_dev, logp_old_dev, adv_dev, n, idx_dev, m, adv_moments_dev,
                       clip_ratio, mu_old_dev, mu_out_dev, logp_out_dev, grad_dev, summary_dev, scratch_dev, ctrl_dev,
                       stream);
}

extern "C" int cf2_ppo_value_grad(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, const float* target_dev,
                                  uint32_t n, const uint32_t* idx_dev, uint32_t m, float* val_out_dev, float* grad_dev,
                                  double* summary_dev, void* scratch_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (m == 0) return CF2_OK;
    if (!weights_dev || !obs_dev || !target_dev || !summary_dev || !scratch_dev || n == 0 || (!idx_dev && m > n))
        return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(obs_dev, 8) || misaligned(target_dev, 4) || misaligned(idx_dev, 4) ||
        misaligned(val_out_dev, 4) || misaligned(grad_dev, 4) || misaligned(summary_dev, 8) || misaligned(scratch_dev, 8))
        return CF2_ERR_INVALID_ARG;
    PpoArgs a = {weights_dev, obs_dev, nullptr, nullptr, target_dev, idx_dev, nullptr, nullptr, nullptr, val_out_dev,
                 nullptr, nullptr, n, m, 0.0f, nullptr};
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? ppo_launch<34, false>(a, grad_dev, summary_dev, scratch_dev, s)
                         : ppo_launch<42, false>(a, grad_dev, summary_dev, scratch_dev, s);
}

// ---- populations (include/cf2sim.h: "for a population of `members` independent learners")
extern "C" size_t cf2_ppo_pop_scratch_bytes(uint32_t members, uint32_t m, uint32_t obs_dim) {
    if ((obs_dim != 34 && obs_dim != 42) || members == 0) return 0;
    return (size_t)members * ppo_pop_slice_bytes(m, obs_dim);
}

// a member stride in elements of `elem` bytes that breaks the alignment `a` of its array
static bool stride_misaligned(size_t stride, size_t elem, size_t a) { return (stride * elem) % a != 0; }

extern "C" int cf2_ppo_policy_grad_pop(uint32_t members, const float* weights_dev, size_t weights_stride, uint32_t obs_dim,
                                       const float* obs_dev, size_t obs_stride, const float* act_dev, size_t act_stride,
                                       const float* logp_old_dev, size_t logp_old_stride, const float* adv_dev,
                                       size_t adv_stride, uint32_t n, const uint32_t* idx_dev, size_t idx_stride, uint32_t m,
                                       const double* adv_moments_dev, const float* clip_ratio_dev, const float* mu_old_dev,
                                       size_t mu_old_stride, float* mu_out_dev, size_t mu_out_stride, float* logp_out_dev,
                                       size_t logp_out_stride, float* grad_dev, double* summary_dev, void* scratch_dev,
                                       const uint32_t* ctrl_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (m == 0 || members == 0) return CF2_OK;
    if (!weights_dev || !obs_dev || !act_dev || !logp_old_dev || !adv_dev || !clip_ratio_dev || !summary_dev ||
        !scratch_dev || n == 0 || (!idx_dev && m > n))
        return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(obs_dev, 8) || misaligned(act_dev, 16) || misaligned(logp_old_dev, 4) ||
        misaligned(adv_dev, 4) || misaligned(idx_dev, 4) || misaligned(adv_moments_dev, 8) || misaligned(clip_ratio_dev, 4) ||
        misaligned(mu_old_dev, 4) || misaligned(mu_out_dev, 4) || misaligned(logp_out_dev, 4) || misaligned(grad_dev, 4) ||
        misaligned(summary_dev, 8) || misaligned(scratch_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (stride_misaligned(obs_stride, 4, 8) || stride_misaligned(act_stride, 4, 16)) return CF2_ERR_INVALID_ARG;
    if (ppo_pop_grid_overflows(members, m, obs_dim)) return CF2_ERR_INVALID_ARG;
    PpoPopArgs p = {};
    p.base = {weights_dev, obs_dev, act_dev, logp_old_dev, adv_dev, idx_dev, adv_moments_dev, mu_old_dev, mu_out_dev,
              logp_out_dev, nullptr, nullptr, n, m, 0.0f, ctrl_dev};
    p.clip = clip_ratio_dev;
    p.s_w = weights_stride, p.s_obs = obs_stride, p.s_act = act_stride, p.s_logp_old = logp_old_stride;
    p.s_adv = adv_stride, p.s_idx = idx_stride, p.s_mu_old = mu_old_stride, p.s_mu_out = mu_out_stride;
    p.s_logp_out = logp_out_stride;
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? ppo_pop_launch<34, true>(p, members, grad_dev, summary_dev, scratch_dev, s)
                         : ppo_pop_launch<42, true>(p, members, grad_dev, summary_dev, scratch_dev, s);
}

extern "C" int cf2_ppo_value_grad_pop(uint32_t members, const float* weights_dev, size_t weights_stride, uint32_t obs_dim,
                                      const float* obs_dev, size_t obs_stride, const float* target_dev, size_t target_stride,
                                      uint32_t n, const uint32_t* idx_dev, size_t idx_stride, uint32_t m, float* val_out_dev,
                                      size_t val_out_stride, float* grad_dev, double* summary_dev, void* scratch_dev,
                                      const uint32_t* ctrl_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (m == 0 || members == 0) return CF2_OK;
    if (!weights_dev || !obs_dev || !target_dev || !summary_dev || !scratch_dev || n == 0 || (!idx_dev && m > n))
        return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(obs_dev, 8) || misaligned(target_dev, 4) || misaligned(idx_dev, 4) ||
        misaligned(val_out_dev, 4) || misaligned(grad_dev, 4) || misaligned(summary_dev, 8) || misaligned(scratch_dev, 8) ||
        misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (stride_misaligned(obs_stride, 4, 8)) return CF2_ERR_INVALID_ARG;
    if (ppo_pop_grid_overflows(members, m, obs_dim)) return CF2_ERR_INVALID_ARG;
    PpoPopArgs p = {};
    p.base = {weights_dev, obs_dev, nullptr, nullptr, target_dev, idx_dev, nullptr, nullptr, nullptr, val_out_dev,
              nullptr, nullptr, n, m, 0.0f, ctrl_dev};
    p.s_w = weights_stride, p.s_obs = obs_stride, p.s_adv = target_stride, p.s_idx = idx_stride;
    p.s_logp_out = val_out_stride;
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? ppo_pop_launch<34, false>(p, members, grad_dev, summary_dev, scratch_dev, s)
                         : ppo_pop_launch<42, false>(p, members, grad_dev, summary_dev, scratch_dev, s);
}

extern "C" int cf2_ppo_fisher_vec(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, uint32_t n,
                                  const uint32_t* idx_dev, uint32_t m, const float* vec_dev, float* out_dev,
                                  double* summary_dev, void* scratch_dev, const uint32_t* ctrl_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (m == 0) return CF2_OK;
    if (!weights_dev || !obs_dev || !vec_dev || !out_dev || !summary_dev || !scratch_dev || n == 0 || (!idx_dev && m > n))
        return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(obs_dev, 8) || misaligned(idx_dev, 4) || misaligned(vec_dev, 4) ||
        misaligned(out_dev, 4) || misaligned(summary_dev, 8) || misaligned(scratch_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    FisherArgs a = {weights_dev, vec_dev, obs_dev, idx_dev, nullptr, nullptr, n, m, ctrl_dev};
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? fisher_launch<34>(a, out_dev, summary_dev, scratch_dev, s)
                         : fisher_launch<42>(a, out_dev, summary_dev, scratch_dev, s);
}

extern "C" int cf2_ppo_fisher_vec_pop(uint32_t members, const float* weights_dev, size_t weights_stride, uint32_t obs_dim,
                                      const float* obs_dev, size_t obs_stride, uint32_t n, const uint32_t* idx_dev,
                                      size_t idx_stride, uint32_t m, const float* vec_dev, size_t vec_stride,
                                      float* out_dev, size_t out_stride, double* summary_dev, void* scratch_dev,
                                      const uint32_t* ctrl_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (m == 0 || members == 0) return CF2_OK;
    if (!weights_dev || !obs_dev || !vec_dev || !out_dev || !summary_dev || !scratch_dev || n == 0 || (!idx_dev && m > n))
        return CF2_ERR_INVALID_ARG;
    if (misaligned(weights_dev, 4) || misaligned(obs_dev, 8) || misaligned(idx_dev, 4) || misaligned(vec_dev, 4) ||
        misaligned(out_dev, 4) || misaligned(summary_dev, 8) || misaligned(scratch_dev, 8) || misaligned(ctrl_dev, 4))
        return CF2_ERR_INVALID_ARG;
    if (stride_misaligned(obs_stride, 4, 8)) return CF2_ERR_INVALID_ARG;
    if (ppo_pop_grid_overflows(members, m, obs_dim)) return CF2_ERR_INVALID_ARG;
    FisherPopArgs p = {};
    p.base = {weights_dev, vec_dev, obs_dev, idx_dev, nullptr, nullptr, n, m, ctrl_dev};
    p.s_w = weights_stride, p.s_v = vec_stride, p.s_obs = obs_stride, p.s_idx = idx_stride;
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? fisher_pop_launch<34>(p, members, out_dev, out_stride, summary_dev, scratch_dev, s)
                         : fisher_pop_launch<42>(p, members, out_dev, out_stride, summary_dev, scratch_dev, s);
}

// ---- rank partials (include/cf2sim.h: "Data-parallel updates")
extern "C" size_t cf2_ppo_partial_doubles(uint32_t obs_dim) {
    return obs_dim == 34 ? ppo_partial_doubles<34>() : obs_dim == 42 ? ppo_partial_doubles<42>() : 0;
}

extern "C" int cf2_ppo_policy_partial(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, const float* act_dev,
                                      const float* logp_old_dev, const float* adv_dev, uint32_t n, const uint32_t* idx_dev,
                                      uint32_t m, const double* adv_moments_dev, const double* moments_count_dev, float clip_ratio,
                                      const float* mu_old_dev, float* mu_out_dev, float* logp_out_dev, int with_grad,
                                      double* partial_dev, void* scratch_dev, const uint32_t* ctrl_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (!partial_dev || misaligned(partial_dev, 8) || misaligned(ctrl_dev, 4)) return CF2_ERR_INVALID_ARG;
    if (m != 0) {
        if (!weights_dev || !obs_dev || !act_dev || !logp_old_dev || !adv_dev || !scratch_dev || n == 0 ||
            (!idx_dev && m > n) || (adv_moments_dev && !moments_count_dev))
            return CF2_ERR_INVALID_ARG;
        if (misaligned(weights_dev, 4) || misaligned(obs_dev, 8) || misaligned(act_dev, 16) || misaligned(logp_old_dev, 4) ||
            misaligned(adv_dev, 4) || misaligned(idx_dev, 4) || misaligned(adv_moments_dev, 8) || misaligned(moments_count_dev, 8) ||
            misaligned(mu_old_dev, 4) || misaligned(mu_out_dev, 4) || misaligned(logp_out_dev, 4) || misaligned(scratch_dev, 8))
            return CF2_ERR_INVALID_ARG;
    }
    PpoArgs a = {weights_dev, obs_dev, act_dev, logp_old_dev, adv_dev, idx_dev, adv_moments_dev, mu_old_dev, mu_out_dev,
                 logp_out_dev, nullptr, nullptr, n, m, clip_ratio, ctrl_dev};
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? ppo_partial_launch<34, true>(a, with_grad != 0, moments_count_dev, partial_dev, scratch_dev, s)
                         : ppo_partial_launch<42, true>(a, with_grad != 0, moments_count_dev, partial_dev, scratch_dev, s);
}

extern "C" int cf2_ppo_value_partial(const float* weights_dev, uint32_t obs_dim, const float* obs_dev,
                                     const float* target_dev, uint32_t n, const uint32_t* idx_dev, uint32_t m,
                                     float* val_out_dev, int with_grad, double* partial_dev, void* scratch_dev,
                                     const uint32_t* ctrl_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (!partial_dev || misaligned(partial_dev, 8) || misaligned(ctrl_dev, 4)) return CF2_ERR_INVALID_ARG;
    if (m != 0) {
        if (!weights_dev || !obs_dev || !target_dev || !scratch_dev || n == 0 || (!idx_dev && m > n))
            return CF2_ERR_INVALID_ARG;
        if (misaligned(weights_dev, 4) || misaligned(obs_dev, 8) || misaligned(target_dev, 4) || misaligned(idx_dev, 4) ||
            misaligned(val_out_dev, 4) || misaligned(scratch_dev, 8))
            return CF2_ERR_INVALID_ARG;
    }
    PpoArgs a = {weights_dev, obs_dev, nullptr, nullptr, target_dev, idx_dev, nullptr, nullptr, nullptr, val_out_dev,
                 nullptr, nullptr, n, m, 0.0f, ctrl_dev};
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? ppo_partial_launch<34, false>(a, with_grad != 0, nullptr, partial_dev, scratch_dev, s)
                         : ppo_partial_launch<42, false>(a, with_grad != 0, nullptr, partial_dev, scratch_dev, s);
}

extern "C" int cf2_ppo_fisher_partial(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, uint32_t n,
                                      const uint32_t* idx_dev, uint32_t m, const float* vec_dev, double* partial_dev,
                                      void* scratch_dev, const uint32_t* ctrl_dev, void* stream) {
    if (obs_dim != 34 && obs_dim != 42) return CF2_ERR_UNSUPPORTED;
    if (!partial_dev || misaligned(partial_dev, 8) || misaligned(ctrl_dev, 4)) return CF2_ERR_INVALID_ARG;
    if (m != 0) {
        if (!weights_dev || !obs_dev || !vec_dev || !scratch_dev || n == 0 || (!idx_dev && m > n)) return CF2_ERR_INVALID_ARG;
        if (misaligned(weights_dev, 4) || misaligned(obs_dev, 8) || misaligned(idx_dev, 4) || misaligned(vec_dev, 4) ||
            misaligned(scratch_dev, 8))
            return CF2_ERR_INVALID_ARG;
    }
    FisherArgs a = {weights_dev, vec_dev, obs_dev, idx_dev, nullptr, nullptr, n, m, ctrl_dev};
    const hipStream_t s = (hipStream_t)stream;
    return obs_dim == 34 ? fisher_partial_launch<34>(a, partial_dev, scratch_dev, s)
                         : fisher_partial_launch<42>(a, partial_dev, scratch_dev, s);
}
