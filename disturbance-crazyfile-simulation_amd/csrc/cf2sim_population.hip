// cf2sim_population.hip -- the fused actor-critic forward (cf2sim_policy.hip) for a population:
// P members with their own packed weight blocks and noise seeds, member m owning rows
// [m * n, (m + 1) * n) of one observation batch, all in one launch.
//
// At the sizes one learner trains at (4 096 - 32 768 rows) cf2_policy_forward is a latency chain:
// P learners pay it P times.  Here each 512-thread block serves exactly one member -- it stages
// that member's fragments into LDS once and runs only that member's 16-row chunks -- so the grid
// is P small policy grids side by side.  Inside its member a block is policy_kernel's MODE 0 with
// member-local numbers: wave w of the member's `bpm` blocks runs the member's chunks w, w + 8 bpm,
// ..., a chunk never straddles members (chunks are counted from the member's first row, the last
// one may be ragged), and the noise drawn once per four trips is shared by ds_bpermute as there.
//
// Identity: the arithmetic of a row is the device functions of cf2sim_policy.h on that row's
// observation, the member's fragments and Philox(seeds[m], counter, row_offset + global row), in
// the same source expressions under the same contraction flags (cf2sim/build.py), and no row's
// result depends on which wave or trip computes it (tests/test_policy_gae_edges.py holds
// policy_kernel to that).  So member m's rows equal
//   cf2_policy_forward(packed + m * stride, n, ..., obs + m n D, seeds[m], counter, row_offset + m n, ...)
// bit for bit (tests/test_population_gpu.py).
#include "cf2sim_policy.h"

namespace cf2 {

template <int D, int PREC>
__global__ void __launch_bounds__(PB, POLICY_WAVES) policy_pop_kernel(const float* __restrict__ Wp, size_t stride,
                                                                          uint32_t n, uint32_t bpm,
                                                                          const float* __restrict__ obs,
                                                                          const uint64_t* __restrict__ seeds,
                                                                          uint32_t counter, uint32_t row_offset, int sample,
                                                                          float* __restrict__ act, float* __restrict__ val,
                                                                          float* __restrict__ logp) {
    using P = Packed<D, PREC>;
    __shared__ __align__(16) float s_w[P::TOTAL];
    // the block's member and its place among the member's blocks (uniform: scalar registers)
    const uint32_t member = blockIdx.x / bpm, lb = blockIdx.x - member * bpm;
    const size_t row0 = (size_t)member * n;        // the member's first global row
    Wp += (size_t)member * stride;
    obs += row0 * D;                               // D even: the member's rows stay 8-B aligned
    act += row0 * 4;
    val += row0;
    if (logp) logp += row0;
    const uint64_t seed = seeds[member];
    const uint32_t key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
    row_offset += (uint32_t)row0;                  // the noise key's row: row_offset + global row (mod 2^32)
    const uint32_t nchunks = (n + CHUNK - 1) / CHUNK;
    const uint32_t wave = lb * PW + (threadIdx.x >> 6), nwaves = bpm * PW;
    {
        const float4* src = reinterpret_cast<const float4*>(Wp);
        float4* dst = reinterpret_cast<float4*>(s_w);
        for (int k = threadIdx.x; k < P::TOTAL / 4; k += PB) dst[k] = src[k];
    }
    __syncthreads();
    const int l = threadIdx.x & 63, r16 = l & 15, g = l >> 4;
    PolicyLane<D, PREC> C;
    policy_lane_init<D, PREC>(s_w + P::O_BIAS, g, C);
    ObsRegs<D, PREC> X;
    if (wave < nchunks) load_obs<D, PREC>(obs, n, wave * CHUNK, l, X);
    // sampling noise as in policy_kernel: at every 4th trip lane group g draws the rows of the
    // wave's chunk of trip k + g, and trip k + j takes its rows' normals from lane group j
    static_assert(RT == 1, "the shared noise draw serves one row tile per chunk");
    float ep[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t kk = 0;
    for (uint32_t c = wave; c < nchunks; c += nwaves, ++kk) {
        if (sample && (kk & 3u) == 0u) {
            const uint32_t cg = c + (uint32_t)g * nwaves;
            if (cg < nchunks) policy_noise(key0, key1, counter, row_offset + cg * CHUNK + (uint32_t)r16, ep);
        }
        const uint32_t r0 = c * CHUNK;
        // an opaque offset keeps the loop-invariant fragment reads inside the loop (policy_kernel)
        int off = 0;
        asm volatile("" : "+v"(off));
        const float* sw = s_w + off;
        ObsRegs<D, PREC> Xc = X;
        policy_standardize<D, PREC>(sw + P::O_BIAS, g, C, Xc);
        if (c + nwaves < nchunks) load_obs<D, PREC>(obs, n, (c + nwaves) * CHUNK, l, X);
        f4v o[RT];
        policy_layers<D, PREC, 0>(sw, sw + P::O_BIAS, sw + P::O_L3, l, Xc, o);
        float e[4];
        const int src = (int)((((kk & 3u) << 4) | (uint32_t)r16) << 2);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(ep[k])));
        const uint32_t row = r0 + (uint32_t)r16;
        if (row < n) policy_emit_eps<D, PREC, 0>(o[0], row, g, C, e, sample, act, val, logp, nullptr);
    }
}

// Blocks per member: what policy_grid gives the member's rows alone, capped by the member's share
// of the 2-blocks-per-CU persistent grid, at least one (members > 2 CUs: one block each, more
// blocks than are resident).  0: the arguments are rejected or nothing would be launched.
static uint32_t pop_blocks(uint32_t members, uint32_t rows) {
    if (members == 0 || rows == 0 || (uint64_t)members * rows > 0xFFFFFFFFull) return 0;
    const uint32_t want = (rows + PW * CHUNK - 1) / (PW * CHUNK);
    if (want == 1) return 1;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint32_t share = 2u * (uint32_t)cus / members;
    const uint32_t b = want < share ? want : share;
    return b ? b : 1u;
}

}  // namespace cf2

using namespace cf2;

template <int D, int PREC>
static int pop_launch(const float* packed_dev, size_t stride, uint32_t members, uint32_t n, uint32_t bpm,
                      const float* obs_dev, const uint64_t* seeds_dev, uint32_t counter, uint32_t row_offset, int sample,
                      float* act_dev, float* val_dev, float* logp_dev, hipStream_t s) {
    hipLaunchKernelGGL((policy_pop_kernel<D, PREC>), dim3(members * bpm), dim3(PB), 0, s, packed_dev, stride, n, bpm,
                       obs_dev, seeds_dev, counter, row_offset, sample, act_dev, val_dev, logp_dev);
    return hipGetLastError() == hipSuccess ? CF2_OK : CF2_ERR_HIP;
}

extern "C" uint32_t cf2_policy_pop_blocks(uint32_t members, uint32_t rows_per_member) {
    const uint32_t b = pop_blocks(members, rows_per_member);
    return (uint64_t)members * b > 0x7FFFFFFFull ? 0u : b;       // the grid is one-dimensional
}

extern "C" int cf2_policy_forward_pop(const float* packed_dev, size_t packed_stride, uint32_t members,
                                      uint32_t rows_per_member, uint32_t obs_dim, int precision, const float* obs_dev,
                                      const uint64_t* seeds_dev, uint32_t counter, uint32_t row_offset, int sample,
                                      float* act_dev, float* val_dev, float* logp_dev, void* stream) {
    if (!packed_dev || !obs_dev || !seeds_dev || !act_dev || !val_dev) return CF2_ERR_INVALID_ARG;
    const size_t packed = cf2_policy_packed_count(obs_dim, precision);
    if (packed == 0) return CF2_ERR_UNSUPPORTED;
    if (((uintptr_t)obs_dev & 7u) || ((uintptr_t)act_dev & 15u) || ((uintptr_t)packed_dev & 15u) ||
        ((uintptr_t)seeds_dev & 7u))
        return CF2_ERR_INVALID_ARG;
    if (members == 0 || packed_stride < packed || (packed_stride & 3u)) return CF2_ERR_INVALID_ARG;
    if (rows_per_member == 0) return CF2_OK;
    const uint32_t bpm = cf2_policy_pop_blocks(members, rows_per_member);
    if (bpm == 0) return CF2_ERR_INVALID_ARG;                     // the rows (or the blocks) do not fit 32 bits
    const hipStream_t s = (hipStream_t)stream;
#define CF2_POP_CASE(D_, P_)                                                                                   \
    if (obs_dim == D_ && precision == P_)                                                                      \
        return pop_launch<D_, P_>(packed_dev, packed_stride, members, rows_per_member, bpm, obs_dev, seeds_dev, \
                                  counter, row_offset, sample, act_dev, val_dev, logp_dev, s);
    CF2_POP_CASE(34, CF2_POLICY_F32)
    CF2_POP_CASE(34, CF2_POLICY_BF16X3)
    CF2_POP_CASE(42, CF2_POLICY_F32)
    CF2_POP_CASE(42, CF2_POLICY_BF16X3)
#undef CF2_POP_CASE
    return CF2_ERR_UNSUPPORTED;
}
