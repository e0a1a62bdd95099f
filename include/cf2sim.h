/*
 * cf2sim.h -- C ABI of the MI355X-native batched CrazyFlie hover environment.
 *
 * One context owns N independent hover environments whose state lives in HBM as
 * structure-of-arrays.  Every entry point is asynchronous on the caller's HIP stream;
 * every I/O buffer is a caller-owned DEVICE pointer.  Return value: 0 on success or a
 * negative cf2_status; the library never aborts the process.
 *
 * Reference interfaces replaced (paths relative to the reference repository root,
 * phoenix_drone_simulation/ omitted):
 *   cf2_reset  <- DroneBaseEnv.reset                         envs/base.py:420-464
 *                 + task_specific_reset                       envs/hover_free.py:237-289, envs/hover.py:204-256
 *                 + apply_domain_randomization                envs/base.py:241-298
 *                 + RandomHJ level redraw (Boltzmann)         envs/hover_free.py:492-536, envs/utils.py:27-39
 *   cf2_step   <- DroneBaseEnv.step and its adversary overrides
 *                                                             envs/base.py:466-507, envs/hover_free.py:391-444,
 *                                                             :778-835, :950-1007; envs/hover.py:649-702, ...
 *                 (one call = aggregate_phy_steps x PybulletPhysicsWithAdversary.step_forward
 *                  envs/physics.py:213-250 / PyBulletPhysics.step_forward :91-124 /
 *                  SimplePhysics.step_forward :130-200, then compute_history/reward/info/done,
 *                  then gym TimeLimit(max_episode_steps) and auto-reset)
 *   cf2_hj_disturbance <- distur_gener                        adversarial_generation/FasTrack_data/distur_gener.py:19-183
 *                         (+ Grid.get_index                   adversarial_generation/odp/Grid/GridProcessing.py:52-71)
 *   cf2_get_state / cf2_set_state: SoA snapshot (the reference never checkpoints env state;
 *                 used for parity tests and checkpoint/resume of rollouts).
 */
#ifndef CF2SIM_H
#define CF2SIM_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF2SIM_ABI_VERSION 8

typedef enum cf2_status {
    CF2_OK = 0,
    CF2_ERR_INVALID_ARG = -1,   /* null pointer, bad enum, inconsistent sizes */
    CF2_ERR_OUT_OF_MEMORY = -2, /* hipMalloc failed */
    CF2_ERR_HIP = -3,           /* a HIP runtime call failed (see cf2_last_hip_error) */
    CF2_ERR_UNSUPPORTED = -4,   /* configuration outside what the kernels implement */
    CF2_ERR_NO_TABLE = -5       /* HJ disturbance requested but no value table bound */
} cf2_status;

/* physics plugin (envs/physics.py) */
enum { CF2_PHYS_BULLET = 0,   /* PyBulletPhysics / PybulletPhysicsWithAdversary: rigid-body restatement of the
                                 btMultiBody step (bullet3 3.21) the reference delegates to stepSimulation() */
       CF2_PHYS_SIMPLE = 1 }; /* SimplePhysics: explicit Euler on rpy (envs/physics.py:130-200) */

/* task (reward / done / reset flavour) */
enum { CF2_TASK_HOVER = 0,       /* DroneHoverBaseEnv  envs/hover.py:16-256 */
       CF2_TASK_HOVER_FREE = 1 };/* DroneHoverFreeEnv  envs/hover_free.py:17-289 */

/* disturbance source (the dstb argument of PybulletPhysicsWithAdversary.step_forward) */
enum { CF2_DSTB_NONE = 0,      /* dstb = (0,0,0)                       hover_free.py:814 */
       CF2_DSTB_EXTERNAL = 1,  /* caller passes dstb[N,3] each step     (test / custom adversary hook) */
       CF2_DSTB_UNIFORM = 2,   /* dstb_space.sample() each env-step    hover_free.py:986, hover.py:1244 */
       CF2_DSTB_CONST = 3,     /* per-episode constant torque ("constant wind", BASELINE config 2) */
       CF2_DSTB_GUST = 4,      /* Philox-driven torque bursts (BASELINE config 4, build-defined) */
       CF2_DSTB_HJ = 5 };      /* HJ bang-bang disturbance from a 15^6 value table  distur_gener.py:19-183 */

/* how the per-episode disturbance level is chosen (HJ / const / gust magnitudes) */
enum { CF2_LEVEL_FIXED = 0,      /* env.disturbance_level constant, e.g. 1.5 (hover_free.py:319) */
       CF2_LEVEL_BOLTZMANN = 1 };/* Boltzmann() redraw at the end of every reset (hover_free.py:536) */

/* 8 Mi envs per context: the state SoA (104 x 4 B x N) must stay addressable by one 32-bit
   buffer-descriptor range; shard larger populations over several contexts / GPUs. */
#define CF2_MAX_ENVS_PER_CTX  (1u << 23)
#define CF2_HJ_PTS 15               /* grid points per dimension, distur_gener.py:179 */
#define CF2_NUM_LEVELS_MAX 32

typedef struct cf2_config {
    /* ---- sizes / plumbing ---- */
    uint32_t num_envs;             /* envs owned by this context (this rank's shard)             */
    uint32_t env_id_offset;        /* global id of env 0 (rank shard offset): RNG keys use global ids */
    uint64_t seed;                 /* Philox4x32-10 key                                            */

    /* ---- env flavour ---- */
    int32_t physics;               /* CF2_PHYS_*                                                   */
    int32_t task;                  /* CF2_TASK_*                                                   */
    int32_t disturbance;           /* CF2_DSTB_*                                                   */
    int32_t level_mode;            /* CF2_LEVEL_*                                                  */
    int32_t aggregate_phy_steps;   /* physics sub-steps per env-step (2)       base.py:35          */
    int32_t obs_rate;              /* sim_freq // observation_frequency (2)    base.py:106          */
    int32_t buf_size;              /* latency ring length int(latency//dt) (2) agents.py:180        */
    int32_t use_latency;           /* agents.py:165                                                */
    int32_t use_motor_dynamics;    /* agents.py:196                                                */
    int32_t max_episode_steps;     /* gym TimeLimit (500)  __init__.py; 0 = none                    */
    int32_t auto_reset;            /* reset envs on done/truncation inside cf2_step                 */
    int32_t enable_reset_distribution; /* base.py:38                                                */
    int32_t observation_noise_on;  /* observation_noise > 0                    hover_free.py:170    */
    int32_t domain_randomization_on; /* domain_randomization > 0               base.py:261          */
    double  domain_randomization;  /* DR factor (0.10)                                              */
    double  motor_thrust_noise;    /* OU sigma = 0.2 * this                    agents.py:206        */

    /* ---- time ---- */
    double sim_freq;               /* Hz (200 bullet, 100 simple)                                  */
    double time_step;              /* 1/sim_freq (nominal; DR redraws per env)                      */

    /* ---- robot constants (URDF + agents.py:142-206) ---- */
    double mass, arm, thrust2weight, ixx, iyy, izz;
    double drag_xy, drag_z;
    double gravity_agent;          /* 9.81  agents.py:145 (K formula)          */
    double gravity_world;          /* 9.81  bc.setGravity base.py:192 / SimplePhysics G physics.py:16 */
    double motor_time_constant;    /* 0.080 */
    double ft0, ft1;               /* FORCE_TORQUE_FACTOR_0/1  agents.py:142-143 */
    double K, A, B;                /* nominal MAX_THRUST, 1 - Ts/T, Ts/T */
    double hover_x, hover_action;  /* sqrt(1/t2w), 2/t2w - 1 */
    double prop_mass, prop_inertia;/* cf21x_bullet.urdf m1..m4_link: 1e-9 kg, 1e-9 kg m^2 */
    double prop_xy, prop_z;        /* prop joint origins (+-0.028, +-0.028, 0.0108) */
    double prop_speed_gain;        /* setJointMotorControl2 targetVelocity = x*100  agents.py:327 */
    double lin_damping, ang_damping;   /* btMultiBody default 0.04 / 0.04 */
    double max_coord_velocity;     /* btMultiBody m_maxCoordinateVelocity 100 */

    /* ---- initial state / reset distribution (hover_free.py:237-289) ---- */
    double init_xyz[3];
    double reset_pos_lim, reset_angle_lim, reset_yaw_lim, reset_vel_lim, reset_rate_lim, reset_yaw_rate_lim;
    double action_init_std, motor_init_std;   /* 0.02, 0.02 */

    /* ---- sensor noise (envs/sensors.py:17-134) & gyro LPF (base.py:107) ---- */
    double pos_norm_std, pos_unif_range, vel_norm_std, vel_unif_range;
    double rot_norm_std, rot_unif_range;
    double gyro_noise_density, gyro_random_walk, gyro_bias_corr_time, gyro_turn_on_bias_sigma;
    double lpf_gain, lpf_ratio;    /* K, T_s/T */

    /* ---- reward / done / cost (hover.py:102-202, hover_free.py:124-235,449-461) ---- */
    double penalty_action, penalty_angle, penalty_spin, penalty_terminal, penalty_velocity, penalty_z;
    double penalty_arp;            /* self.ARP */
    double penalty_dist;           /* 1 for DroneHoverBaseEnv (-dist term), 0 for free */
    double target_pos[3], target_rpy[3], target_rate[3];
    double done_rp_limit;          /* rad: deg2rad(60) or deg2rad(75) */
    double done_rate_limit_deg;    /* 300 or 1000 */
    double done_z_min;             /* 0.2 */
    double cost_xy_lim, cost_z_lim, cost_rp_lim, cost_vel_lim, cost_rate_lim;

    /* ---- disturbance ---- */
    double dstb_level;             /* fixed level (CF2_LEVEL_FIXED) */
    double dstb_umax[3];           /* 5.3e-3, 5.3e-3, 1.43e-4   distur_gener.py:152 */
    double dstb_uniform_hi[3];     /* 1e-3, 1e-3, 1e-4          hover_free.py:315 */
    double gust_onset_prob, gust_max_level;   /* 0.01, 1.5 */
    int32_t gust_duration;         /* 20 env-steps */
    int32_t num_levels;            /* Boltzmann support size (21) */
    double level_values[CF2_NUM_LEVELS_MAX];  /* np.around(energies, 1) */
    double level_cdf[CF2_NUM_LEVELS_MAX];     /* normalised cumsum(p), numpy choice()  */
    double hj_grid_min[6];         /* per-dim lower bounds (Grid.min)                */
    double hj_grid_dx[6];          /* Grid.dx                                       */
    double hj_grid_points[6][CF2_HJ_PTS]; /* np.linspace node values (Grid.grid_points) */

    /* ---- multi-drone envs (BASELINE config 5; no reference code) ----
     * num_drones consecutive envs form one env group of drones flying a formation: drone k sits at
     * init_xyz + ((k/2 - (ceil(num_drones/2)-1)/2) * formation_dx, 0, (k%2) * formation_dz).
     * downwash_on: each drone feels, from every drone j of its group above it (dz > 0, dxy < 10),
     * the downwash force of gym-pybullet-drones BaseAviary._downwash with the URDF coefficients
     * parsed but unused by the reference (agents.py:251-257):
     *   F = dw_coeff_1 (prop_radius / (4 dz))^2 exp(-0.5 (dxy / (dw_coeff_2 dz + dw_coeff_3))^2)
     * along -z of the body (LINK_FRAME), at the centre of mass.  Bullet physics only. */
    int32_t num_drones;            /* 1 (default), 2, 4 or 8; num_envs and env_id_offset multiples of it */
    int32_t downwash_on;
    double dw_coeff[3];            /* 2267.18, 0.16, -0.11 */
    double prop_radius;            /* 2.31348e-2 m */
    double formation_dx, formation_dz;   /* 0.5 m, 1.0 m */

    /* ---- ground effect (BasePhysics.calculate_ground_effect envs/physics.py:27-58, applied in
     * step_forward physics.py:116-120 / 243-246; the reference's envs never enable it;
     * cf2_physics_step only, see cf2_set_ground_effect): while
     * |roll|, |pitch| < pi/2 each prop gets the extra thrust f_i * gnd_eff_coeff *
     * (prop_radius / (4 max(z_i, gnd_eff_h_clip)))^2, z_i = world height of prop i.  Bullet only. */
    int32_t use_ground_effect;
    double gnd_eff_coeff;          /* URDF gnd_eff_coeff 11.36859 */
    double gnd_eff_h_clip;         /* GND_EFF_H_CLIP agents.py:156 */
} cf2_config;

/* SoA layout descriptor returned by cf2_layout(): state_f[field*num_envs + env],
 * state_i[field*num_envs + env]. Field meaning is documented in DESIGN.md. */
typedef struct cf2_layout {
    uint32_t num_envs;
    uint32_t num_float_fields;
    uint32_t num_int_fields;
    uint32_t obs_dim;              /* 34 with observation noise, 42 without */
    uint32_t obs_len;              /* 13 or 17 */
    uint32_t f_pos, f_quat, f_vel, f_omega, f_rpy, f_motor, f_ou, f_abuf, f_bias, f_lpf, f_held,
             f_obs_prev, f_hist_act, f_param, f_dstb;
    uint32_t i_ep_step, i_rng, i_flags, i_level, i_gust;
    uint32_t num_params;           /* per-env DR parameters (19; the motor A[4] = 1 - B[4] is derived) */
    uint32_t f_motor_lo;           /* 4: low words of the motor state (state = f_motor + f_motor_lo) */
} cf2_layout;

typedef struct cf2_ctx cf2_ctx;

int  cf2_abi_version(void);
/* Errors the kernels of ctx recorded on the device (synchronises the device): bit 1 = a helper
 * wave of the small-N kernels gave up waiting for the LDS hand-over of the reset pose (its reset
 * rows would be built from a stale pose; never observed).  clear != 0 resets the word.  The
 * kernels never trap: they record and finish, and the host decides. */
int  cf2_device_errors(cf2_ctx* ctx, uint32_t* flags_out, int clear);
size_t cf2_config_sizeof(void);     /* lets FFI callers check their struct mirror */
const char* cf2_status_string(int status);
int  cf2_last_hip_error(void);

int  cf2_create(const cf2_config* cfg, cf2_ctx** out_ctx);
int  cf2_destroy(cf2_ctx* ctx);
int  cf2_layout_get(const cf2_ctx* ctx, cf2_layout* out);
/* Cache policy of the stores of the large-N one-step kernel (cf2_step / cf2_step_packed above
 * 32 768 envs per context; DESIGN.md section 3, "Store cache policy").  The fused kernels behind
 * cf2_collect_step, cf2_collect_rollout and cf2_rollout have one form (plain state stores, nt
 * observation rows) under every policy.  A policy is three values, each CF2_STORE_PLAIN (write-back), _NT (streamed past the Infinity
 * Cache), _WT (write-through, sc1) or _NT_WT: out3[0] the state stores, out3[1] the observation
 * rows, out3[2] the per-env outputs (rew, done, trunc, cost, level, final_obs).  cf2_create takes it
 * from the environment variable CF2SIM_STORE_POLICY: "auto" (default: chosen from the env count and
 * the bytes an env-step moves), "plain", "wt", "nt", or "state=P,obs=P,out=P" with P one of plain |
 * wt | nt | nt_wt (parts left out keep the plain policy's value).  An unknown value makes cf2_create
 * return CF2_ERR_INVALID_ARG, a policy the library has no kernel instance for CF2_ERR_UNSUPPORTED.
 * Contexts of up to 32 768 envs run kernels with one fixed policy and report that one.
 * cf2_store_policy: what ctx's cf2_step runs.  cf2_store_policy_for: what cf2_create would pick for cfg under
 * `text` (NULL: the environment variable), without touching a device.  Results never depend on it. */
#define CF2_STORE_PLAIN 0
#define CF2_STORE_NT    2
#define CF2_STORE_WT    16
#define CF2_STORE_NT_WT 18
int  cf2_store_policy(const cf2_ctx* ctx, uint32_t* out3);
int  cf2_store_policy_for(const cf2_config* cfg, const char* text, uint32_t* out3);

/* Bind HJ value tables: V_dev = [num_tables][15^6] float32 C-order [roll,pitch,yaw,p,q,r]
 * (the on-disk fastrack_{level}_15x15.npy format).  table_level_index maps Boltzmann level
 * index -> table row (or -1 = no table, dstb 0).  Caller owns V_dev for the ctx lifetime.
 * Binding derives, once, the disturbance sign bits of every grid node (the distur_gener rule over
 * the node's 7 value taps, distur_gener.py:155-183; 1 byte per node, 11.4 MB per table, owned by
 * the ctx): the env-step gathers one byte per env.  Rebind after changing the table contents.
 * Synchronous and device-wide: waits for all work on the device first (V_dev may have been
 * written on any stream; steps in flight may still read the previous tables), then derives the
 * bits.  On failure the ctx keeps its previous binding, or has none (CF2_ERR_NO_TABLE on the
 * next HJ step) if the previous bits were already overwritten.  num_tables * 15^6 must fit in
 * 32 bits (at most 377 tables). */
int  cf2_bind_hj_tables(cf2_ctx* ctx, const float* V_dev, int num_tables,
                        const int32_t* table_of_level /* host, num_levels entries */);

/* The distribution the per-episode disturbance level is drawn from (CF2_LEVEL_BOLTZMANN contexts;
 * CF2_ERR_UNSUPPORTED otherwise): p_host[k] >= 0 is the weight of level_values[k], count ==
 * num_levels.  The reference fixes it to Boltzmann() (envs/utils.py:27-39) and registers its
 * "...WithCurriculumHJAdversary" id with that same distribution; this is the hook a curriculum
 * sets its own through.  The CDF is built as numpy's choice(p=...) builds it: cumulative sum in
 * double, divided by its last entry; the draw is unchanged (the count of CDF entries <= u, u in
 * [0, 1)), so a level of weight 0 is never drawn.  A wrong count, a negative or non-finite entry
 * or a sum that is not positive and finite: CF2_ERR_INVALID_ARG, nothing changed.  The CDF goes
 * into the context's config and only its words of the device tables are uploaded (the device
 * error word stays).  Synchronous and device-wide, as cf2_bind_hj_tables: it waits for all work on
 * the device first.  It takes effect from the next reset (cf2_reset or an auto-reset inside a
 * step); running episodes keep their level. */
int  cf2_set_level_distribution(cf2_ctx* ctx, const double* p_host, int32_t count);

/* Reset envs whose mask byte is non-zero (mask_dev NULL = all), write their obs rows. */
int  cf2_reset(cf2_ctx* ctx, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* One env-step for all envs.  act_dev [N,4] (16-B aligned); dstb_dev [N,3] (only for CF2_DSTB_EXTERNAL,
 * else NULL); obs_dev [N,obs_dim] (8-B aligned; 16-B stores where it is 16-B aligned); rew_dev [N]; done_dev [N] (terminal OR truncated, gym 4-tuple semantics);
 * trunc_dev [N] (TimeLimit truncation, may be NULL); cost_dev [N] (may be NULL);
 * level_dev [N] disturbance level of the finished step (may be NULL);
 * final_obs_dev [N,obs_dim] pre-reset observation of envs that auto-reset this step (may be NULL). */
int  cf2_step(cf2_ctx* ctx, const float* act_dev, const float* dstb_dev,
              float* obs_dev, float* rew_dev, uint8_t* done_dev, uint8_t* trunc_dev,
              float* cost_dev, float* level_dev, float* final_obs_dev, void* stream);

/* One physics sub-step of every env, without the env-step around it: the physics plugin's
 * step_forward (PyBulletPhysics.step_forward physics.py:91-124, SimplePhysics :130-200,
 * PybulletPhysicsWithAdversary.step_forward :213-250; plugin construction envs/base.py:223-232):
 * apply_action (latency ring, PWM, OU thrust noise, motor dynamics), motor forces + yaw torque,
 * adversary torques dstb[0], dstb[1] (dstb_dev [N,3] or NULL = none), drag, the rigid-body step
 * and update_information.  No observation, reward, TimeLimit or auto-reset.  time_step > 0
 * overrides every env's dt for this call (BasePhysics.set_parameters physics.py:60-68); <= 0
 * uses the per-env dt (domain randomisation).  act_dev [N,4] 16-B aligned. */
int  cf2_physics_step(cf2_ctx* ctx, const float* act_dev, const float* dstb_dev, float time_step, void* stream);
/* Ground effect on / off for this context's Bullet physics (the physics object's
 * use_ground_effect, envs/physics.py:18-25); the initial value is cfg.use_ground_effect.
 * It applies to cf2_physics_step only: the reference's envs build their physics with the default
 * use_ground_effect=False (envs/base.py:223-232), so the env-step kernels carry no ground-effect
 * code and cf2_step / cf2_rollout return CF2_ERR_UNSUPPORTED while it is on.
 * Returns CF2_ERR_UNSUPPORTED for SimplePhysics contexts. */
int  cf2_set_ground_effect(cf2_ctx* ctx, int on);

/* K consecutive env-steps fused in one launch (rollout mode; SURVEY section 7 "fused K-step"):
 * the env state stays in registers across the K steps.  Step k reads actions act_dev + k *
 * act_stride_elems ([N,4], 16-B aligned, stride a multiple of 4) and writes the k-th [N, ...]
 * slab of every output: obs_dev [K,N,obs_dim] (8-B aligned), rew_dev [K,N], done_dev [K,N] and,
 * when not NULL, trunc_dev [K,N], cost_dev [K,N], level_dev [K,N], final_obs_dev [K,N,obs_dim].
 * Results are identical to K cf2_step calls with the same actions (the reference's
 * IWPGAlgorithm.roll_out loop algs/iwpg/iwpg.py:372-410 with actions known in advance, e.g.
 * open-loop or random-action rollouts).  Not for CF2_DSTB_EXTERNAL envs (CF2_ERR_UNSUPPORTED). */
int  cf2_rollout(cf2_ctx* ctx, int K, const float* act_dev, size_t act_stride_elems,
                 float* obs_dev, float* rew_dev, uint8_t* done_dev, uint8_t* trunc_dev,
                 float* cost_dev, float* level_dev, float* final_obs_dev, void* stream);

/* Whole-state snapshot (device buffers sized by cf2_layout). */
int  cf2_get_state(const cf2_ctx* ctx, float* state_f_dev, int32_t* state_i_dev, void* stream);
int  cf2_set_state(cf2_ctx* ctx, const float* state_f_dev, const int32_t* state_i_dev, void* stream);

/* Stand-alone batched distur_gener: states_dev [n,6] = [roll,pitch,yaw,p,q,r] (float32),
 * V_dev one 15^6 table, out dstb_dev [n,3] = opt_d, out uopt_dev [n,3] = opt_u (may be NULL). */
int  cf2_hj_disturbance(const cf2_config* cfg, const float* V_dev, const float* states_dev,
                        uint32_t n, float level, float* dstb_dev, float* uopt_dev, void* stream);

/* ---- batched rollout caller ----
 * Gaussian MLP actor-critic forward of the reference's PPO networks for a batch of observations,
 * one fused launch on the matrix cores: ActorCritic.step (algs/core.py:371-395), MLPGaussianActor
 * (core.py:228-291) pi D->50->50->4 ReLU, MLPCritic D->64->64->1 tanh (algs/ppo/defaults.py:8-13).
 * fp32 activations and accumulation; products in one of two precisions:
 *   CF2_POLICY_F32     exact fp32 (v_mfma_f32_16x16x4_f32, the result of an fmaf chain over k);
 *   CF2_POLICY_BF16X3  split-bf16 operands (x = hi + lo, three bf16 MFMAs per product block):
 *                      <= ~1.1e-5 relative error per product, ~5x the fp32 rate.
 * Weights: the flat block (cf2_policy_weights_count(D) floats; layout in csrc/cf2sim_policy.hip:
 * input-major matrices, pi then v, log_std after the pi head) is converted once per weight update
 * by cf2_policy_pack into the packed block (cf2_policy_packed_count(D, precision) floats, 16-B
 * aligned: MFMA operand fragments in the kernel's order) that the forward calls take with the
 * same precision.
 * obs_dev [n, D] (D = 34 or 42, 8-B aligned); sample != 0: act = mu + exp(log_std) * eps,
 * eps ~ N(0,1) from Philox keyed (seed, counter, row + row_offset); else act = mu.  Outputs
 * act_dev [n,4] (16-B aligned), val_dev [n], logp_dev [n] (sum of Normal log-densities; may be
 * NULL). */
enum cf2_policy_precision { CF2_POLICY_F32 = 0, CF2_POLICY_BF16X3 = 1 };
size_t cf2_policy_weights_count(uint32_t obs_dim);
size_t cf2_policy_packed_count(uint32_t obs_dim, int precision);
int  cf2_policy_pack(const float* weights_dev, uint32_t obs_dim, int precision, float* packed_dev, void* stream);
int  cf2_policy_forward(const float* packed_dev, uint32_t n, uint32_t obs_dim, int precision, const float* obs_dev,
                        uint64_t seed, uint32_t counter, uint32_t row_offset, int sample,
                        float* act_dev, float* val_dev, float* logp_dev, void* stream);
/* Value of the rows with mask_dev[r] != 0 only (time-out bootstraps V(final obs)); other rows of
 * val_dev are left untouched. */
int  cf2_value_forward_masked(const float* packed_dev, uint32_t n, uint32_t obs_dim, int precision,
                              const float* obs_dev, const uint8_t* mask_dev, float* val_dev, void* stream);

/* cf2_policy_forward for a population of independent learners in one launch
 * (csrc/cf2sim_population.hip).  `members` packed blocks lie packed_stride floats apart
 * (packed_stride >= cf2_policy_packed_count(obs_dim, precision), a multiple of 4; packed_dev 16-B
 * aligned); member m owns rows [m * rows_per_member, (m + 1) * rows_per_member) of obs_dev
 * [members * rows_per_member, D] and of act_dev / val_dev / logp_dev, and its sampling noise is
 * Philox keyed (seeds_dev[m], counter, row_offset + global row); seeds_dev [members] is device memory,
 * 8-B aligned.  Member m's rows are bit for bit those of
 *   cf2_policy_forward(packed_dev + m * packed_stride, rows_per_member, ..., obs_dev + m * rows_per_member * D,
 *                      seeds[m], counter, row_offset + m * rows_per_member, ...).
 * Each 512-thread block serves one member, cf2_policy_pop_blocks(members, rows_per_member) blocks per
 * member: max(1, min(ceil(rows_per_member / 128), floor(2 CUs / members))); 0 for arguments the
 * forward rejects or launches nothing for.  A NULL pointer other than logp_dev, a misaligned pointer
 * (obs_dev, seeds_dev 8 bytes; act_dev, packed_dev 16), members == 0, a packed_stride below the packed
 * count or no multiple of 4, members * rows_per_member >= 2^32 or a grid of 2^31 or more blocks:
 * CF2_ERR_INVALID_ARG; an (obs_dim, precision) without a kernel: CF2_ERR_UNSUPPORTED;
 * rows_per_member == 0: CF2_OK, nothing launched.  Every error returns before anything is launched. */
int  cf2_policy_forward_pop(const float* packed_dev, size_t packed_stride, uint32_t members, uint32_t rows_per_member,
                            uint32_t obs_dim, int precision, const float* obs_dev, const uint64_t* seeds_dev,
                            uint32_t counter, uint32_t row_offset, int sample, float* act_dev, float* val_dev,
                            float* logp_dev, void* stream);
uint32_t cf2_policy_pop_blocks(uint32_t members, uint32_t rows_per_member);

/* One step of the collect loop in one launch: the env-step of cf2_step (act_dev -> obs_dev, rew,
 * done, trunc, final_obs; same arguments, no disturbance tensor, no cost/level outputs), then
 * cf2_policy_forward(sample = 1) on the new observations -> act_out_dev [N,4] (16-B aligned, the
 * next env-step's actions; must not be act_dev), val_out_dev [N], logp_out_dev [N].  Replaces the
 * pair env.step + ac.step of IWPGAlgorithm.roll_out (phoenix_drone_simulation/algs/iwpg/iwpg.py:
 * 377-380; ActorCritic.step algs/core.py:371-395).  Every output is bit-identical to the two
 * calls.  Fused only where built (precision CF2_POLICY_BF16X3, obs_dim 34 = sensor noise on, the
 * default Bullet env-step shape, one drone per formation; any N); elsewhere it returns
 * CF2_ERR_UNSUPPORTED and launches nothing, and the caller makes the two calls. */
int  cf2_collect_step(cf2_ctx* ctx, const float* act_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev,
                      uint8_t* trunc_dev, float* final_obs_dev, const float* packed_dev, uint32_t obs_dim,
                      int precision, uint64_t seed, uint32_t counter, uint32_t row_offset, float* act_out_dev,
                      float* val_out_dev, float* logp_out_dev, void* stream);

/* K steps of the collect loop: env-step k (actions act_dev + k*N*4) and then the policy forward +
 * sampling on its observations (noise counter counter + k), whose actions the next env-step
 * takes.  N <= 32768 (C2, the 8-GPU node shard): one launch, the env state in registers for the K
 * steps (64-env groups with helper waves computing the auto-resets, as cf2_step there); larger N:
 * one cf2_collect_step launch per step (faster there than a one-launch loop).  Buffers, slab-major:
 * act_dev [K+1,N,4] (slab 0 in: the first step's actions; slabs 1..K out), val_dev / logp_dev
 * [K+1,N] (slabs 1..K out, slab 0 untouched), obs_dev [K,N,obs_dim] (slab k = the observation
 * after env-step k), rew_dev / done_dev [K,N], trunc_dev / final_obs_dev [K,N] / [K,N,obs_dim]
 * or NULL.  Every output is bit-identical to K cf2_collect_step calls with act_out = the next
 * slab and counters counter, counter + 1, ... (IWPGAlgorithm.roll_out's loop,
 * phoenix_drone_simulation/algs/iwpg/iwpg.py:372-410, ActorCritic.step algs/core.py:371-395).
 * Built where cf2_collect_step is (else CF2_ERR_UNSUPPORTED, nothing launched). */
int  cf2_collect_rollout(cf2_ctx* ctx, int K, float* act_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev,
                         uint8_t* trunc_dev, float* final_obs_dev, const float* packed_dev, uint32_t obs_dim,
                         int precision, uint64_t seed, uint32_t counter, uint32_t row_offset, float* val_dev,
                         float* logp_dev, void* stream);

/* cf2_collect_step / cf2_collect_rollout with the env-step's info outputs: cost_dev and level_dev
 * ([N] for the step, [K, N] slab-major for the rollout; either may be NULL) receive what cf2_step
 * writes there, info['cost'] of compute_info (envs/hover_free.py:138-166) and the disturbance
 * level of the finished step (the level column of the reference's episodic_data.csv).  With both
 * NULL the calls are the two above, which are these with NULL, NULL: same kernels, same bits. */
int  cf2_collect_step_info(cf2_ctx* ctx, const float* act_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev,
                           uint8_t* trunc_dev, float* final_obs_dev, const float* packed_dev, uint32_t obs_dim,
                           int precision, uint64_t seed, uint32_t counter, uint32_t row_offset, float* act_out_dev,
                           float* val_out_dev, float* logp_out_dev, float* cost_dev, float* level_dev, void* stream);
int  cf2_collect_rollout_info(cf2_ctx* ctx, int K, float* act_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev,
                              uint8_t* trunc_dev, float* final_obs_dev, const float* packed_dev, uint32_t obs_dim,
                              int precision, uint64_t seed, uint32_t counter, uint32_t row_offset, float* val_dev,
                              float* logp_dev, float* cost_dev, float* level_dev, void* stream);

/* Batched GAE over [T, n] rollout buffers (algs/core.py:459-535 finish_path on every env's
 * episode slices): done/trunc uint8 (terminal -> bootstrap 0, time-out -> trunc_val), the end of
 * the buffer bootstraps last_val [n].  rew_den > 0: reward scaling, delta uses
 * clip(r / rew_den, -10, 10) with rew_den = ret_oms.std + 1e-5 (core.py:522-529); <= 0: none.
 * Outputs adv [T, n], ret = adv + val [T, n] and, if disc_ret_dev is not NULL, the per-episode
 * discounted returns of the unscaled rewards (core.py:519, the return statistics' input). */
int  cf2_gae(uint32_t T, uint32_t n, const float* rew_dev, const float* val_dev, const uint8_t* done_dev,
             const uint8_t* trunc_dev, const float* trunc_val_dev, const float* last_val_dev, float gamma,
             float lam, float rew_den, float* adv_dev, float* ret_dev, float* disc_ret_dev, void* stream);

/* Episode statistics over [T, n] rollout buffers (algs/iwpg/iwpg.py:372-410: roll_out keeps ep_ret,
 * ep_costs and ep_len and stores EpRet / EpLen / EpCosts at every episode end; the epoch log prints
 * their mean, std, min and max).  The envs auto-reset on the device and an episode outlasts a
 * collect, so the running sums are per-env carries (carry_ret f32, carry_cost f32, carry_len int32,
 * [n] each, updated in place; zero them where an episode is abandoned).  Per step t, in time order:
 * carry_ret += rew[t], carry_cost += cost[t] (cost_dev NULL: 0), ++carry_len, plain f32 / int adds;
 * where done[t] != 0 (terminal or time-out) the episode ends including step t: its three values go
 * to slot [t, env] of the optional ep_*_out buffers ([T, n]; other slots are left untouched) and
 * into the summary, and the carry restarts at 0.  summary_dev, 16 doubles: [0] episodes finished,
 * [1..4] return sum, sum of squares, min, max, [5..8] length, [9..12] cost, [13..15] 0; with no
 * episode min = +inf and max = -inf.  accumulate != 0 merges this call into the summary already
 * there (one whose count is 0 is empty whatever else it holds); 0 overwrites.  scratch_dev:
 * cf2_episode_stats_scratch_bytes(n) bytes, 8-byte aligned.  Two launches on `stream`; no atomics,
 * the same input gives the same bits.  T == 0 or n == 0: CF2_OK, nothing launched. */
size_t cf2_episode_stats_scratch_bytes(uint32_t n);
int  cf2_episode_stats(uint32_t T, uint32_t n, const float* rew_dev, const float* cost_dev, const uint8_t* done_dev,
                       float* carry_ret_dev, float* carry_cost_dev, int32_t* carry_len_dev, float* ep_ret_out_dev,
                       int32_t* ep_len_out_dev, float* ep_cost_out_dev, double* summary_dev, int accumulate,
                       void* scratch_dev, void* stream);

/* Per-level episode outcomes over [T, n] rollout buffers: cf2_episode_stats with the finished
 * episodes binned by the disturbance level they ran under and split into crashes and time-outs.
 * The reference logs the level with every episode (episodic_data.csv: episode, disturbance level,
 * steps, return, written by the logger of algs/iwpg/iwpg.py) and evaluates a policy per level
 * (utils/evaluation.py).  The scan and the carries are cf2_episode_stats': per step t, in time
 * order, carry_ret += rew[t], carry_cost += cost[t] (cost_dev NULL: 0), ++carry_len, plain f32 /
 * int adds; where done[t] != 0 the episode ends including step t and the carries restart at 0, so
 * splitting [T, n] over several calls changes no carry and no episode value.
 * Bin: the episode goes to row k of the table where level_dev[t, env] (the level of the finished
 * step, as cf2_step writes it) has the bits of level_values_dev[k] (the first such k), to row L
 * ("other") where none has, and to row 0 with level_dev NULL.  1 <= L <= CF2_NUM_LEVELS_MAX.
 * Quota: with episodes_left_dev ([n] int32) an episode that ends in env e is recorded only while
 * episodes_left[e] > 0, and the word is then decremented; the carries restart either way.  A
 * quota of E per env makes an evaluation count exactly E episodes of every env, however short.
 * table_dev, [L + 1][16] doubles: words [0..12] of a row as the cf2_episode_stats summary (count;
 * sum, sum of squares, min, max of return, length, cost), [13] crashes (done and not trunc), [14]
 * time-outs (trunc != 0), both 0 with trunc_dev NULL, [15] 0; an empty row has count 0, min +inf,
 * max -inf.  accumulate != 0 merges this call into each row already there (a row whose count is 0
 * is empty whatever else it holds); 0 overwrites.  scratch_dev:
 * cf2_level_outcomes_scratch_bytes(T, n, L) bytes (0 for arguments the call rejects or ignores),
 * 8-byte aligned.  Three launches on `stream`; no atomics, the geometry depends on (T, n, L) only
 * and the same input gives the same bits.  L == 0 or L > 32, a NULL required pointer (rew, done,
 * level_values, the carries, table, scratch) or a misaligned pointer (4 bytes; 8 for table and
 * scratch): CF2_ERR_INVALID_ARG; T == 0 or n == 0: CF2_OK, nothing launched or written.  Every
 * error returns before anything is launched. */
size_t cf2_level_outcomes_scratch_bytes(uint32_t T, uint32_t n, uint32_t L);
int  cf2_level_outcomes(uint32_t T, uint32_t n, const float* rew_dev, const float* cost_dev, const uint8_t* done_dev,
                        const uint8_t* trunc_dev, const float* level_dev, const float* level_values_dev, uint32_t L,
                        float* carry_ret_dev, float* carry_cost_dev, int32_t* carry_len_dev,
                        int32_t* episodes_left_dev, double* table_dev, int accumulate, void* scratch_dev,
                        void* stream);

/* Column moments of a dense row-major [rows, D] f32 matrix, 1 <= D <= 64, read once: out_dev gets
 * mean[D], then M2[D] = sum over rows of (x - mean)^2, in fp64 -- the batch moments the running
 * statistics (utils/online_mean_std.py; update_running_statistics, iwpg.py:412-420) are updated
 * from.  Sums are fp64 and shifted by a row of the matrix, block partials (count, mean, M2) are
 * merged in index order (Chan et al.): M2 >= 0, exactly 0 for a constant column, and the same input
 * gives the same bits.  x_dev is 4-byte aligned; a 16-byte (8-byte) aligned one streams with
 * 16-byte (8-byte) loads, whatever D.  scratch_dev:
 * cf2_column_moments_scratch_bytes(rows, D) bytes, 8-byte aligned.  D == 0 or D > 64:
 * CF2_ERR_INVALID_ARG; rows == 0: CF2_OK, nothing launched or written. */
size_t cf2_column_moments_scratch_bytes(uint64_t rows, uint32_t D);
int  cf2_column_moments(const float* x_dev, uint64_t rows, uint32_t D, double* out_dev, void* scratch_dev,
                        void* stream);

/* Loss and gradient of the PPO update (algs/ppo/ppo.py compute_loss_pi without the entropy term,
 * which is constant in the trained parameters: log_std has requires_grad=False; and the critic's mean
 * squared error of algs/iwpg/iwpg.py), one fused launch per network plus a merge launch.
 * weights_dev is the flat block of cf2_policy_pack's input (cf2_policy_weights_count(obs_dim) floats),
 * not the packed one: the optimiser owns the flat values and grad_dev comes back in that layout.
 * obs_dim 34 or 42; the observation is standardised as in the forward, (obs - mean) * scale.
 * Rows: obs [n, obs_dim] (8-byte aligned), act [n, 4] (16-byte aligned), logp_old, adv, target [n].
 * idx_dev: m row indices, each < n, repeats allowed (a value mini-batch); NULL: rows 0..m-1, m <= n.
 * Policy, per selected row j: mu = pi(z), logp = sum_k -((a_k - mu_k) / sigma_k)^2 / 2 - log sigma_k
 * - log(2 pi) / 2, ratio = exp(logp - logp_old), L_j = -min(ratio A, clamp(ratio, 1 - c, 1 + c) A),
 * loss = mean L_j.  A = adv, or with adv_moments_dev ({mean, M2} over the n advantages, as
 * cf2_column_moments(adv, n, 1, ...) writes them) A = (adv - mean) / (sqrt(M2 / n) + 1e-8), in fp64
 * and rounded to fp32: the standardisation of the reference's buffer get().  d L_j / d logp is
 * -A ratio where the unclipped term is the minimum or the ratio is inside the clip range, else 0;
 * ReLU' is 0 at a pre-activation <= 0.  mu_old_dev [n, 4] (optional) enables the exact Gaussian KL,
 * KL_j = sum_k (mu_old_k - mu_k)^2 / (2 sigma_k^2).  Value: v = V(z), loss = mean (v - target)^2.
 * Optional outputs, dense by position j: mu_out [m, 4], logp_out [m], val_out [m].
 * grad_dev: the policy call writes exactly the words [P_W1, P_LOGSTD) of the flat layout (pi W1 b1
 * W2 b2 W3 b3), the value call exactly [V_W1, O_MEAN) (v W1 b1 W2 b2 W3 b3); every other word is
 * left untouched.  NULL: evaluate only (no backward pass), same summary bits.
 * summary_dev, 8 doubles.  Policy: [0] m, [1] loss, [2] mean(logp_old - logp), [3] share of rows
 * with |ratio - 1| > c, [4] mean exact KL (0 without mu_old), [5] mean ratio, [6..7] 0.  Value: [0] m,
 * [1] loss, rest 0.
 * Products are exact fp32 (v_mfma_f32_16x16x4_f32 and fmaf).  Block partials go to scratch_dev
 * (cf2_ppo_scratch_bytes(m, obs_dim) bytes, 8-byte aligned; 0 for an unsupported obs_dim) and are
 * merged in block-index order in fp64, divided by m and rounded once: no atomics, the same input
 * gives the same bits.  obs_dim not 34 or 42: CF2_ERR_UNSUPPORTED; m == 0: CF2_OK, nothing launched
 * or written; a NULL required pointer (weights, the row inputs, summary, scratch), a misaligned
 * pointer, n == 0 or idx_dev == NULL with m > n: CF2_ERR_INVALID_ARG.  Every error returns before
 * anything is launched. */
size_t cf2_ppo_scratch_bytes(uint32_t m, uint32_t obs_dim);
int  cf2_ppo_policy_grad(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, const float* act_dev,
                         const float* logp_old_dev, const float* adv_dev, uint32_t n, const uint32_t* idx_dev,
                         uint32_t m, const double* adv_moments_dev, float clip_ratio, const float* mu_old_dev,
                         float* mu_out_dev, float* logp_out_dev, float* grad_dev, double* summary_dev,
                         void* scratch_dev, void* stream);
int  cf2_ppo_value_grad(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, const float* target_dev,
                        uint32_t n, const uint32_t* idx_dev, uint32_t m, float* val_out_dev, float* grad_dev,
                        double* summary_dev, void* scratch_dev, void* stream);

/* cf2_ppo_policy_grad behind a gate, for an update loop that never returns to the host: ctrl_dev is
 * the control block of cf2_adam_step (below).  NULL, or ctrl_dev[0] == 0 when the kernels start:
 * exactly cf2_ppo_policy_grad, the same bits in every output.  ctrl_dev[0] != 0: both launches return
 * at once; grad, summary, mu_out, logp_out and the scratch are left untouched.  The launches only read
 * the word.  Errors as cf2_ppo_policy_grad; ctrl_dev is 4-byte aligned. */
int  cf2_ppo_policy_grad_gated(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, const float* act_dev,
                               const float* logp_old_dev, const float* adv_dev, uint32_t n, const uint32_t* idx_dev,
                               uint32_t m, const double* adv_moments_dev, float clip_ratio, const float* mu_old_dev,
                               float* mu_out_dev, float* logp_out_dev, float* grad_dev, double* summary_dev,
                               void* scratch_dev, const uint32_t* ctrl_dev, void* stream);

/* One optimiser step on a slice of the flat weight block, one launch: torch.optim.Adam with its
 * defaults (no amsgrad, no weight decay) preceded by torch.nn.utils.clip_grad_norm_ (the reference
 * clips the actor's and the critic's gradients before the optimiser step), and the stop rule of
 * update_policy_net (algs/iwpg/iwpg.py: `if kl > target_kl: break`) applied on the device.
 * weights, grad, exp_avg and exp_avg_sq are whole flat blocks in the layout of cf2_policy_pack's
 * input; the call reads the words [begin, begin + count) of grad, reads and writes the same words of
 * the other three and touches nothing else.  step_dev: one uint32, the optimiser's step count (on
 * the device, so that a skipped call does not advance it).  ctrl_dev (optional): four uint32, zeroed
 * by the caller when an update starts: [0] stop flag, [1] steps applied under this block, [2..3]
 * reserved, left 0.
 *   1. ctrl_dev[0] != 0: return, nothing is written.
 *   2. ctrl_dev and kl_summary_dev given and kl_summary_dev[4] (the mean exact KL of a policy
 *      summary) > (double)target_kl: ctrl_dev[0] = 1, nothing else is written.  The comparison is
 *      strict and false for a NaN, as the reference's.
 *   3. otherwise t = ++*step_dev; norm = sqrt(sum g^2) over the slice; with max_grad_norm > 0
 *      g = g min(1, max_grad_norm / (norm + 1e-6)) (grad_dev itself is never written);
 *      m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2;
 *      w = w - lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps); ++ctrl_dev[1];
 *      *norm_out_dev (optional) = norm, the norm before clipping that torch's function returns.
 * The hyper-parameters are the fp32 values passed (0.999f, not 0.999).  The norm, the bias
 * corrections and every word's update are evaluated in fp64 and rounded once into the fp32 state;
 * non-finite gradients get no special case.  One workgroup, no atomics, sums in a fixed order: the
 * same input gives the same bits, and nothing but this launch writes the stop flag.
 * count == 0: CF2_OK, nothing launched; a NULL weights, grad, exp_avg, exp_avg_sq or step pointer, a
 * misaligned pointer (4 bytes; 8 for norm_out and kl_summary), begin + count past 32 bits, lr
 * negative or not finite: CF2_ERR_INVALID_ARG; count > 2^20: CF2_ERR_UNSUPPORTED.  Every error
 * returns before anything is launched. */
int  cf2_adam_step(float* weights_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                   uint32_t begin, uint32_t count, uint32_t* step_dev, float lr, float beta1, float beta2, float eps,
                   float max_grad_norm, double* norm_out_dev, const double* kl_summary_dev, float target_kl,
                   uint32_t* ctrl_dev, void* stream);

/* The three calls above for a population of `members` independent learners (cf2_policy_forward_pop's
 * members), each as one launch chain whose length does not depend on `members`.  The defining
 * property: for every k < members, member k's outputs are the bits the stand-alone call
 * (cf2_ppo_policy_grad_gated, cf2_ppo_value_grad, cf2_adam_step) writes when given base + k * stride
 * for every array argument, clip_ratio_dev[k] (or lr_dev[k], max_grad_norm_dev[k], target_kl_dev[k])
 * and ctrl_dev + 4 k.  Nothing else is written: not the words between the members' slices, not the
 * words of grad outside the network's slice.
 * Every array argument is followed by its member stride in elements of its own type (floats, or
 * uint32 for idx); the strides are independent of one another (in member-major rollout storage obs
 * is [members, T + 1, n, D] and everything else [members, T, n, ...]).  A stride may be anything the
 * member slices do not overlap under; the stride of an optional array that is NULL is ignored.
 * Alignment: what the stand-alone call asks of a pointer holds for the base and for the stride in
 * bytes (obs: 8, act: 16, everything else 4).  n and m are the same for every member.
 *   weights_dev, grad_dev   [members] flat blocks weights_stride floats apart (grad_dev NULL: evaluate only)
 *   idx_dev                 member k's m indices at idx_dev + k * idx_stride; NULL: rows 0..m-1 of every member
 *   adv_moments_dev         [members][2] doubles (NULL: advantages as they are)
 *   clip_ratio_dev          [members] floats, device memory
 *   summary_dev             [members][8] doubles
 *   ctrl_dev                [members][4] uint32 (cf2_adam_step_pop's control blocks) or NULL: ungated.
 *                           A member whose ctrl word [4 k] is non-zero when the kernels start is
 *                           skipped in both launches -- nothing of it is written -- and the other
 *                           members are unaffected.  The value call takes the gate too.
 *   scratch_dev             cf2_ppo_pop_scratch_bytes(members, m, obs_dim) bytes, 8-byte aligned:
 *                           `members` slices of cf2_ppo_scratch_bytes(m, obs_dim) rounded up to 16
 *                           bytes.  0 for an unsupported obs_dim or members == 0.
 * Geometry: member k runs the blocks it runs alone, b = min(ceil(ceil(m / 16) / 4), 512) of them, as
 * blocks [k b, (k + 1) b) of one grid of members * b; the merge launch has one grid row per member.
 * No atomics; the same input gives the same bits.
 * cf2_adam_step_pop: one 1 024-thread workgroup per member on the words [begin, begin + count) of
 * member k's blocks (weights, grad, exp_avg, exp_avg_sq: block_stride floats apart); step_dev
 * [members] uint32; norm_out_dev [members] doubles or NULL; kl_summary_dev [members][8] doubles or
 * NULL; ctrl_dev [members][4] uint32 or NULL; lr_dev [members] floats (every value finite and >= 0:
 * the caller's duty, the call cannot read them); max_grad_norm_dev [members] floats or NULL (no
 * clipping); target_kl_dev [members] floats, required where ctrl_dev and kl_summary_dev are both
 * given; beta1, beta2 and eps are shared.  Member k's workgroup is the only writer of member k's
 * words (the stop flag among them); the gradient launches only read them.
 * Errors, all returned before anything is launched: obs_dim not 34 or 42: CF2_ERR_UNSUPPORTED (Adam:
 * count > 2^20); a NULL required pointer (those of the stand-alone call, clip_ratio_dev, lr_dev), a
 * misaligned base or stride, n == 0, idx_dev == NULL with m > n, a grid of 2^31 blocks or more
 * (members * b; Adam: members), begin + count past 32 bits: CF2_ERR_INVALID_ARG; m == 0, members == 0
 * or count == 0: CF2_OK, nothing launched or written. */
size_t cf2_ppo_pop_scratch_bytes(uint32_t members, uint32_t m, uint32_t obs_dim);
int  cf2_ppo_policy_grad_pop(uint32_t members, const float* weights_dev, size_t weights_stride, uint32_t obs_dim,
                             const float* obs_dev, size_t obs_stride, const float* act_dev, size_t act_stride,
                             const float* logp_old_dev, size_t logp_old_stride, const float* adv_dev, size_t adv_stride,
                             uint32_t n, const uint32_t* idx_dev, size_t idx_stride, uint32_t m,
                             const double* adv_moments_dev, const float* clip_ratio_dev, const float* mu_old_dev,
                             size_t mu_old_stride, float* mu_out_dev, size_t mu_out_stride, float* logp_out_dev,
                             size_t logp_out_stride, float* grad_dev, double* summary_dev, void* scratch_dev,
                             const uint32_t* ctrl_dev, void* stream);
int  cf2_ppo_value_grad_pop(uint32_t members, const float* weights_dev, size_t weights_stride, uint32_t obs_dim,
                            const float* obs_dev, size_t obs_stride, const float* target_dev, size_t target_stride,
                            uint32_t n, const uint32_t* idx_dev, size_t idx_stride, uint32_t m, float* val_out_dev,
                            size_t val_out_stride, float* grad_dev, double* summary_dev, void* scratch_dev,
                            const uint32_t* ctrl_dev, void* stream);
int  cf2_adam_step_pop(uint32_t members, float* weights_dev, const float* grad_dev, float* exp_avg_dev,
                       float* exp_avg_sq_dev, size_t block_stride, uint32_t begin, uint32_t count, uint32_t* step_dev,
                       const float* lr_dev, float beta1, float beta2, float eps, const float* max_grad_norm_dev,
                       double* norm_out_dev, const double* kl_summary_dev, const float* target_kl_dev,
                       uint32_t* ctrl_dev, void* stream);

/* Fisher-vector product of the policy, out = F vec, for the natural-gradient updates (algs/npg,
 * algs/trpo: the Hessian-vector product of the mean KL to the detached policy).  The policy is
 * Gaussian with an untrained log_std, so KL = sum_k (mu_old_k - mu_k)^2 / (2 sigma_k^2) and its Hessian
 * at mu = mu_old is exactly the Gauss-Newton matrix F = (1/m) sum_rows J^T Sigma^-1 J (J = d mu / d
 * parameters; the term with the network's second derivatives is multiplied by mu - mu_old = 0).  One
 * fused launch (the primal forward, a tangent pass J vec, dout = J vec / sigma^2, the backward pass
 * and gradient GEMMs of cf2_ppo_policy_grad) plus the merge launch.  No damping is added.
 * weights_dev: the flat block, obs_dim 34 or 42; obs [n, obs_dim] (8-byte aligned); idx_dev / m as in
 * the gradient calls (the reference takes every fourth row, obs[::4]: idx = 0, 4, 8, ...).
 * vec_dev and out_dev are whole flat blocks: the call reads the words [P_W1, P_LOGSTD) of vec and
 * writes exactly those words of out; every other word is left untouched.  ReLU' is 0 at a
 * pre-activation <= 0.  summary_dev, 8 doubles: [0] m, [1] vec^T F vec = mean_rows sum_k (J vec)_k^2 /
 * sigma_k^2 accumulated in fp64, [2..7] 0.  ctrl_dev: the gate of cf2_ppo_policy_grad_gated (NULL or
 * ctrl_dev[0] == 0: run; otherwise both launches return at once and out, summary and the scratch are
 * left untouched).  scratch_dev: cf2_ppo_scratch_bytes(m, obs_dim) bytes, 8-byte aligned.  Products
 * are exact fp32, block partials are merged in block-index order in fp64, divided by m and rounded
 * once: no atomics, the same input gives the same bits.  obs_dim not 34 or 42: CF2_ERR_UNSUPPORTED;
 * m == 0: CF2_OK, nothing launched or written; a NULL weights, obs, vec, out, summary or scratch
 * pointer, a misaligned pointer, n == 0 or idx_dev == NULL with m > n: CF2_ERR_INVALID_ARG.  Every
 * error returns before anything is launched. */
int  cf2_ppo_fisher_vec(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, uint32_t n,
                        const uint32_t* idx_dev, uint32_t m, const float* vec_dev, float* out_dev,
                        double* summary_dev, void* scratch_dev, const uint32_t* ctrl_dev, void* stream);

/* cf2_ppo_fisher_vec for a population of `members` independent learners: it replaces `members`
 * cf2_ppo_fisher_vec calls (two launches each) by two launches in all, under the contract of the
 * population gradient calls above.  For every k < members, member k's out words and summary are the
 * bits cf2_ppo_fisher_vec writes when given weights_dev + k weights_stride, obs_dev + k obs_stride,
 * idx_dev + k idx_stride, vec_dev + k vec_stride, out_dev + k out_stride, summary_dev + 8 k and
 * ctrl_dev + 4 k.  Nothing else is written: not the words between the members' slices, not the words
 * of out outside [P_W1, P_LOGSTD).  Member k runs the grid it has alone, b = min(ceil(ceil(m / 16) /
 * 4), 512) blocks, as blocks [k b, (k + 1) b) of one grid of members * b (one kernel body serves both
 * forms); the merge is the population gradient calls'.  No atomics; the same input gives the same bits.
 *   idx_dev      read-only.  idx_stride == 0: one list of m indices that every member reads (the
 *                updaters' every-fourth-row list).  cf2_ppo_policy_grad_pop and cf2_ppo_value_grad_pop
 *                add k * idx_stride in the same way, so a zero stride means a shared list there too;
 *                they are unchanged.  NULL: rows 0..m-1 of every member.
 *   summary_dev  [members][8] doubles
 *   ctrl_dev     [members][4] uint32 or NULL: ungated.  A member whose word [4 k] is non-zero is skipped
 *                in both launches -- its out, summary and scratch slice stay as they are -- and no
 *                other member reads that word.
 *   scratch_dev  cf2_ppo_pop_scratch_bytes(members, m, obs_dim) bytes, 8-byte aligned, sliced as the
 *                population gradient calls slice it.
 * Errors, all returned before anything is launched: obs_dim not 34 or 42: CF2_ERR_UNSUPPORTED; m == 0
 * or members == 0: CF2_OK, nothing launched or written; a NULL weights, obs, vec, out, summary or
 * scratch pointer, a misaligned base (4 bytes; 8 for obs, summary and scratch), an odd obs_stride, n ==
 * 0, idx_dev == NULL with m > n, a grid of 2^31 blocks or more: CF2_ERR_INVALID_ARG. */
int  cf2_ppo_fisher_vec_pop(uint32_t members, const float* weights_dev, size_t weights_stride, uint32_t obs_dim,
                            const float* obs_dev, size_t obs_stride, uint32_t n, const uint32_t* idx_dev,
                            size_t idx_stride, uint32_t m, const float* vec_dev, size_t vec_stride, float* out_dev,
                            size_t out_stride, double* summary_dev, void* scratch_dev, const uint32_t* ctrl_dev,
                            void* stream);

/* Data-parallel updates: the gradient, evaluation and Fisher-vector calls above in two levels, so that
 * the ranks of a node update from all rows.  Level one, per rank: cf2_ppo_policy_partial,
 * cf2_ppo_value_partial and cf2_ppo_fisher_partial run the first launch of cf2_ppo_policy_grad_gated,
 * cf2_ppo_value_grad and cf2_ppo_fisher_vec (the same kernels on the same arguments) and end in a merge
 * that writes, instead of grad and summary, one rank-partial block of cf2_ppo_partial_doubles(obs_dim)
 * doubles (8 + the value slice's words, the larger slice, so one all-gather shape serves the three
 * calls; 0 for an unsupported obs_dim) to partial_dev (8-byte aligned):
 *   [0]     m, the rank's selected rows
 *   [1..7]  the fp64 sums over those rows of the summary slots 1..7 (not divided)
 *   [8 + p] the fp64 sum of word p of the network's slice of the gradient (pi W1 b1 W2 b2 W3 b3, or v
 *           likewise) or of F vec: the block partials summed in block-index order, not divided by m
 *           and not rounded to fp32; the words past the slice, and all of them when with_grad == 0
 *           (evaluate only), are 0.
 * m == 0 is legal: a rank may own no selected row.  Then only partial_dev (and ctrl_dev) are looked
 * at, one launch writes a zeroed block, and the optional outputs are left untouched.
 * moments_count_dev (policy, required with adv_moments_dev; 8-byte aligned): one double on the device,
 * the rows adv_moments_dev was taken over -- all ranks' rows after cf2_moments_combine, whose output
 * block is {count, mean, M2}, not the n rows of this rank -- so that A = (adv - mean) / (sqrt(M2 /
 * count) + 1e-8).  A one-thread launch ahead of the gradient kernel writes {mean, M2 (n / count)} into
 * the scratch for it; with count == n the factor is exactly 1 and the call is
 * cf2_ppo_policy_grad_gated's arithmetic bit for bit.  The count stays on the device so that an update
 * never waits for it.  ctrl_dev: the gate of cf2_ppo_policy_grad_gated (NULL or ctrl_dev[0] == 0: run; otherwise
 * every launch returns at once and nothing is written).  scratch_dev: cf2_ppo_scratch_bytes(m, obs_dim)
 * bytes.  Errors as the single-rank calls, plus a NULL or misaligned partial_dev and adv_moments_dev
 * without moments_count_dev: CF2_ERR_INVALID_ARG.  Every error returns before anything is launched.
 *
 * Level two, on every rank after an all-gather of the blocks: cf2_ppo_reduce reads blocks_dev
 * [world][cf2_ppo_partial_doubles(obs_dim)] in rank order, sums them in that order in fp64, divides by
 * M = sum of the [0] words and rounds once, and writes exactly what the single-rank call writes: the
 * pi (value == 0) or v (value != 0) slice of grad_dev (a whole flat block; NULL: the summary only) and
 * summary_dev, 8 doubles, [0] = M.  One launch, no atomics: the same blocks give the same bits, so
 * every rank holds the same grad and summary.  world == 1 gives the bits of the single-rank call (the
 * same order of sums, one division, one rounding).  Splitting the same rows differently over ranks
 * changes which 16-row tiles share a block's fp32 partial, so the bits differ between splits; each
 * split meets the accuracy rule of the single-rank calls against fp64.  ctrl_dev: the gate, as above.
 * The row counts are on the device: with M == 0 the launch writes nothing.  obs_dim not 34 or 42:
 * CF2_ERR_UNSUPPORTED; world == 0, a NULL blocks_dev or summary_dev, a misaligned pointer (8 bytes; 4 for
 * grad_dev and ctrl_dev): CF2_ERR_INVALID_ARG, before anything is launched. */
size_t cf2_ppo_partial_doubles(uint32_t obs_dim);
int  cf2_ppo_policy_partial(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, const float* act_dev,
                            const float* logp_old_dev, const float* adv_dev, uint32_t n, const uint32_t* idx_dev,
                            uint32_t m, const double* adv_moments_dev, const double* moments_count_dev, float clip_ratio,
                            const float* mu_old_dev, float* mu_out_dev, float* logp_out_dev, int with_grad,
                            double* partial_dev, void* scratch_dev, const uint32_t* ctrl_dev, void* stream);
int  cf2_ppo_value_partial(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, const float* target_dev,
                           uint32_t n, const uint32_t* idx_dev, uint32_t m, float* val_out_dev, int with_grad,
                           double* partial_dev, void* scratch_dev, const uint32_t* ctrl_dev, void* stream);
int  cf2_ppo_fisher_partial(const float* weights_dev, uint32_t obs_dim, const float* obs_dev, uint32_t n,
                            const uint32_t* idx_dev, uint32_t m, const float* vec_dev, double* partial_dev,
                            void* scratch_dev, const uint32_t* ctrl_dev, void* stream);
int  cf2_ppo_reduce(const double* blocks_dev, uint32_t world, uint32_t obs_dim, int value, float* grad_dev,
                    double* summary_dev, const uint32_t* ctrl_dev, void* stream);

/* Batch moments across ranks.  cf2_column_moments_partial is cf2_column_moments writing a rank's
 * moments block {count, mean[D], M2[D]} (1 + 2 D doubles, 8-byte aligned; count = rows) to block_dev;
 * rows == 0 is legal and writes a zeroed block.  cf2_moments_combine folds blocks_dev [world][1 + 2 D]
 * left in rank order, in fp64, with the update of Chan et al. (n = na + nb, delta = mean_b - mean_a,
 * mean = mean_a + delta nb / n, M2 = M2_a + M2_b + delta^2 na nb / n) into out_dev, one block of the same
 * layout.  Blocks of count 0 are skipped and the first block that counts is taken as it stands: world
 * == 1 returns its input bit for bit, and no block counting gives {0, 0.., 0..}.  D = 1 serves the
 * advantages (out_dev + 1 is the adv_moments_dev of cf2_ppo_policy_partial, out_dev its
 * moments_count_dev) and the discounted returns, D = obs_dim the observations.  One launch of one
 * workgroup; the same blocks give the same bits.  D == 0 or D > 64, world == 0, a NULL or misaligned
 * (8 bytes) pointer: CF2_ERR_INVALID_ARG, before anything is launched. */
int  cf2_column_moments_partial(const float* x_dev, uint64_t rows, uint32_t D, double* block_dev, void* scratch_dev,
                                void* stream);
int  cf2_moments_combine(const double* blocks_dev, uint32_t world, uint32_t D, double* out_dev, void* stream);

/* The solver of the natural-gradient updates on a slice [begin, begin + count) of flat blocks, with
 * every scalar on the device: ng_state_dev, CF2_NG_STATE_DOUBLES doubles. */
enum { CF2_NG_RDOTR = 0,        /* r.r of the conjugate-gradient recurrence (cg_init: b.b) */
       CF2_NG_CG_STEPS = 1,     /* cg_step calls applied since cg_init */
       CF2_NG_CG_DONE = 2,      /* 1 once sqrt(r.r) < 1e-10: later cg_step calls write nothing */
       CF2_NG_XHX = 3,          /* direction: x.(F x + damping x) */
       CF2_NG_ALPHA = 4,        /* direction: sqrt(2 target_kl / (xHx + 1e-8)) */
       CF2_NG_EXPECTED = 5,     /* direction: b.step, the expected improvement of the full step */
       CF2_NG_STEP_FRAC = 6,    /* line search: decay^trial of the accepted trial; 0: all rejected */
       CF2_NG_ACCEPT_STEP = 7,  /* line search: accepted trial + 1; 0: all rejected */
       CF2_NG_LOSS_BEFORE = 8,  /* line search: *loss_before_dev */
       CF2_NG_LOSS_AFTER = 9,   /* line search: loss of the accepted trial; all rejected: loss before */
       CF2_NG_KL_AFTER = 10,    /* line search: KL of the accepted trial; all rejected: 0 */
       CF2_NG_PDOTZ = 11,       /* p.(z + damping p) of the last applied cg_step */
       CF2_NG_BDOTB = 12,       /* cg_init: b.b = |grad|^2 over the slice */
       CF2_NG_RESIDUAL = 13,    /* r.r after the last applied cg_step, the converging one included */
       CF2_NG_STATE_DOUBLES = 16 /* 14, 15: reserved, zeroed by cg_init */ };
/* All four calls: one launch of one workgroup that strides over the slice; the vectors (grad, b, x, r,
 * p, z, step, weights, weights_old) are whole flat blocks of which only the words [begin, begin +
 * count) are read or written.  Dot products are fp64 sums of fp64 products of the fp32 words in a
 * fixed order; every written word is evaluated in fp64 from the fp32 values and rounded once; a dot
 * product after an update reads the rounded words.  The scalars passed as float (damping, target_kl,
 * decay) enter as the fp32 values.  No atomics; the same input gives the same bits.  ctrl_dev is the
 * control block of cf2_adam_step; in cg_init, cg_step and direction it is an optional read-only gate
 * (ctrl_dev[0] != 0: return, nothing written).  count == 0: CF2_OK, nothing launched; a NULL pointer
 * (every pointer but the gate is required), a misaligned one (4 bytes; 8 for ng_state, eval_summary
 * and loss_before), begin + count past 32 bits, damping or target_kl negative or not finite, decay
 * outside (0, 1], trial >= total: CF2_ERR_INVALID_ARG; count > 2^20: CF2_ERR_UNSUPPORTED.  Every
 * error returns before anything is launched.
 *
 * cf2_ng_cg_init: b = -grad, x = 0, r = p = b; ng_state: RDOTR = BDOTB = RESIDUAL = b.b, every other
 * word (CG_DONE included) 0.
 *
 * cf2_ng_cg_step, given z = F p (cf2_ppo_fisher_vec of p): if CG_DONE is set, return with nothing
 * written.  z' = z + damping p; a = RDOTR / (p.z' + 1e-6); x += a p; r -= a z'; new = r.r;
 * ++CG_STEPS, RESIDUAL = new, PDOTZ = p.z'; if sqrt(new) < 1e-10: CG_DONE = 1 and p, RDOTR stay;
 * otherwise p = r + new / (RDOTR + 1e-6) p and RDOTR = new.  z' is not stored.
 *
 * cf2_ng_direction, given z = F x: XHX = x.(z + damping x); ALPHA = sqrt(2 target_kl / (XHX + 1e-8));
 * step = ALPHA x; EXPECTED = b.step; weights_old = weights; weights = weights_old + step (trial 0).
 * A negative XHX + 1e-8 gives NaN, as the reference's; there is no special case.
 *
 * cf2_ng_line_search, trial `trial` of `total` (0-based), given the policy summary of the weights of
 * that trial (eval_summary_dev: cf2_ppo_policy_grad_gated with mu_old; [1] loss, [4] KL) and
 * *loss_before_dev (e.g. word 1 of the summary on the starting weights).  ctrl_dev is required.
 *   1. ctrl_dev[0] != 0: return, nothing written.
 *   2. accept iff the loss is finite, loss_before - loss >= 0 and KL <= 1.5 (double)target_kl (a NaN
 *      fails each): ctrl_dev[0] = 1, ctrl_dev[1] = trial + 1, STEP_FRAC = decay^trial, ACCEPT_STEP =
 *      trial + 1, LOSS_BEFORE, LOSS_AFTER = loss, KL_AFTER = KL; the weights stay.
 *   3. rejected and trial + 1 < total: weights = weights_old + decay^(trial + 1) step (the power by
 *      repeated squaring in fp64); nothing else written.
 *   4. the last trial rejected: weights = weights_old bit for bit, STEP_FRAC = ACCEPT_STEP = 0,
 *      KL_AFTER = 0, LOSS_AFTER = LOSS_BEFORE = loss before, ctrl_dev[0] = 1.
 * Nothing but this launch and cf2_adam_step writes the stop flag. */
int  cf2_ng_cg_init(const float* grad_dev, float* b_dev, float* x_dev, float* r_dev, float* p_dev, uint32_t begin,
                    uint32_t count, double* ng_state_dev, const uint32_t* ctrl_dev, void* stream);
int  cf2_ng_cg_step(const float* z_dev, float* x_dev, float* r_dev, float* p_dev, uint32_t begin, uint32_t count,
                    float damping, double* ng_state_dev, const uint32_t* ctrl_dev, void* stream);
int  cf2_ng_direction(const float* z_dev, const float* x_dev, const float* b_dev, float* step_dev, float* weights_dev,
                      float* weights_old_dev, uint32_t begin, uint32_t count, float damping, float target_kl,
                      double* ng_state_dev, const uint32_t* ctrl_dev, void* stream);
int  cf2_ng_line_search(float* weights_dev, const float* weights_old_dev, const float* step_dev, uint32_t begin,
                        uint32_t count, uint32_t trial, uint32_t total, float decay, float target_kl,
                        const double* eval_summary_dev, const double* loss_before_dev, double* ng_state_dev,
                        uint32_t* ctrl_dev, void* stream);

/* The four solver calls for a population of `members` independent learners: each replaces `members`
 * launches of its stand-alone twin (cf2_ng_cg_init, cf2_ng_cg_step, cf2_ng_direction,
 * cf2_ng_line_search) by one launch of one 1 024-thread workgroup per member.  For every k < members,
 * member k's words are the bits the stand-alone call writes when given base + k * block_stride for
 * every flat-block vector (grad, b, x, r, p, z, step, weights, weights_old: block_stride floats apart,
 * as cf2_adam_step_pop takes its blocks), damping_dev[k], target_kl_dev[k], ng_state_dev + 16 k,
 * eval_summary_dev + 8 k, loss_before_dev + k * loss_before_stride (doubles; e.g. word 1 of a
 * [members][8] summary with stride 8) and ctrl_dev + 4 k.  begin, count, trial, total and decay are
 * shared.  The arithmetic is the stand-alone kernels': fp64 dot products in a fixed order, every
 * written word rounded once.  Member k's workgroup is the only writer of member k's state, stop flag
 * and weights and reads no other member's; nothing outside [begin, begin + count) of a member's blocks
 * and nothing between the blocks is written.  A member whose gate word ctrl_dev[4 k] is set (or whose
 * CG_DONE is set, in cg_step) is skipped while the others go on in the same launch.  damping_dev and
 * target_kl_dev are device arrays of `members` floats, every value finite and >= 0: the caller's
 * duty, the call cannot read them.
 * count == 0 or members == 0: CF2_OK, nothing launched; a NULL pointer (every pointer but the gate of
 * cg_init, cg_step and direction is required; cf2_ng_line_search_pop needs ctrl_dev), a misaligned
 * base (4 bytes; 8 for ng_state, eval_summary and loss_before), members >= 2^31, begin + count past 32
 * bits, decay outside (0, 1], trial >= total: CF2_ERR_INVALID_ARG; count > 2^20: CF2_ERR_UNSUPPORTED.
 * Every error returns before anything is launched. */
int  cf2_ng_cg_init_pop(uint32_t members, const float* grad_dev, float* b_dev, float* x_dev, float* r_dev, float* p_dev,
                        size_t block_stride, uint32_t begin, uint32_t count, double* ng_state_dev,
                        const uint32_t* ctrl_dev, void* stream);
int  cf2_ng_cg_step_pop(uint32_t members, const float* z_dev, float* x_dev, float* r_dev, float* p_dev,
                        size_t block_stride, uint32_t begin, uint32_t count, const float* damping_dev,
                        double* ng_state_dev, const uint32_t* ctrl_dev, void* stream);
int  cf2_ng_direction_pop(uint32_t members, const float* z_dev, const float* x_dev, const float* b_dev, float* step_dev,
                          float* weights_dev, float* weights_old_dev, size_t block_stride, uint32_t begin, uint32_t count,
                          const float* damping_dev, const float* target_kl_dev, double* ng_state_dev,
                          const uint32_t* ctrl_dev, void* stream);
int  cf2_ng_line_search_pop(uint32_t members, float* weights_dev, const float* weights_old_dev, const float* step_dev,
                            size_t block_stride, uint32_t begin, uint32_t count, uint32_t trial, uint32_t total,
                            float decay, const float* target_kl_dev, const double* eval_summary_dev,
                            const double* loss_before_dev, size_t loss_before_stride, double* ng_state_dev,
                            uint32_t* ctrl_dev, void* stream);

/* Multi-GPU observation exchange as deltas (the north star's per-step RCCL
 * all-gather of the obs slab).  The reference has no counterpart: its MPI ranks exchange only
 * gradients and statistics (utils/mpi_tools.py:30-44); the rows materialised here are exactly what
 * compute_history (envs/base.py:305-321) returns on every rank.
 * A row is [o_{k-1}, A0, o_k, A1] (obs_len OL = 13 with sensor noise, 17 without); per env-step a
 * rank packs only o_k of every env, a bitmap of the envs that auto-reset and, for up to `cap` of
 * them, the reset row's o_0 and action part, into cf2_obs_packed_words(n, OL, cap) 32-bit words
 * (a multiple of 4).  After an all-gather of the packed buffers ([world][words], rank order,
 * equal shards of n envs) a receiver keeps them and only advances every env's steps since its
 * reset (cf2_obs_consume: age_dev uint16 [world n], saturating; all 0 after the observations came
 * from a full gather right after a reset of every env).  Rows are materialised on request
 * (cf2_obs_rows) from the gathered buffers of step k (capacity cap) and k - 1 (cap_prev), the ages
 * after step k's consume and the actions of steps k, k - 1 and k - 2 (act, act_prev, act_prev2:
 * [world n, 4]); out gets rows [row0, row0 + nrows) as [nrows, 2 OL + 8].  Rank r's packed buffer
 * is at r * stride words (0: cf2_obs_packed_words(n, OL, cap), the all-gather of one step).  Time-out look-ahead:
 * envs whose age becomes watch_age at a consume (max_episode_steps - L; 0xFFFFFFFF: off) are
 * counted per rank into pred_dev[world] (pred_next_dev[world], a different row, is zeroed for the
 * next step): at most that many envs time out L steps later, so the caller can size that step's
 * cap.  Valid under auto-reset for env-step shapes whose action buffer holds only the step's action
 * after a step (aggregate_phy_steps a multiple of buf_size, latency on: the reference's default).
 * Side slots go to 64-env pack blocks, never to single envs (layout and allocation:
 * csrc/cf2sim_pack.h); a block whose resets find no room in the side slab (an overflow) is marked
 * dropped: exactly its reset rows have NaN in their o_0 / A parts, *overflow_dev counts the dropped
 * blocks, every other row and all o_k parts stay exact, and later steps are exact again.  A pack
 * counts spill slots in scratch_dev (PACK_SCRATCH_WORDS = 32 words, zeroed before the pack) and
 * zeroes next_scratch_dev (the counter of the next pack on its stream; or NULL). */
size_t cf2_obs_packed_words(uint32_t n, uint32_t obs_len, uint32_t cap);
int  cf2_obs_pack(const float* obs_dev, const uint8_t* reset_dev, uint32_t n, uint32_t obs_len, uint32_t cap,
                  uint32_t* packed_dev, uint32_t* scratch_dev, uint32_t* next_scratch_dev, void* stream);
/* The env-step (cf2_step's outputs, no final_obs) with the pack of its observations fused in: the
 * env kernel writes packed_dev (cf2_obs_packed_words(N, OL, cap) words) as cf2_obs_pack would, from
 * the rows it has in LDS, so no pack launch re-reads them (step_kernel_small's wave 2 at N <= 32 768,
 * every thread of step_kernel's blocks above), except the 4 informational header words, which it
 * leaves as they are (no receiver reads them).  scratch_dev: this buffer's spill counter
 * (PACK_SCRATCH_WORDS = 32 words), zeroed by the caller before the call (cf2_xchg_* zeroes a
 * batch's counters in the batch's consume, after its packs). */
int  cf2_step_packed(cf2_ctx* ctx, const float* act_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev,
                     uint8_t* trunc_dev, float* cost_dev, float* level_dev, uint32_t* packed_dev, uint32_t* scratch_dev,
                     uint32_t cap, void* stream);
int  cf2_obs_consume(const uint32_t* packed_all_dev, uint32_t world, uint32_t n, uint32_t obs_len, uint32_t cap,
                     uint16_t* age_dev, uint32_t* overflow_dev, uint32_t watch_age, uint32_t* pred_dev,
                     uint32_t* pred_next_dev, void* stream);
int  cf2_obs_rows(const uint32_t* packed_all_dev, uint32_t cap, uint32_t stride, const uint32_t* packed_prev_all_dev,
                  uint32_t cap_prev, uint32_t stride_prev, uint32_t world, uint32_t n, uint32_t obs_len,
                  const uint16_t* age_dev, const float* act_dev, const float* act_prev_dev, const float* act_prev2_dev,
                  uint32_t row0, uint32_t nrows, float* rows_dev, void* stream);

/* The same exchange driven natively: an RCCL communicator of this library's own (one rank per GPU,
 * created on the current device, with an exchange stream of its own) and, per batch of env-steps,
 * one ncclAllGather of the batch's packed buffers and one consume on the exchange stream after the
 * env stream's work so far.  cf2_xchg_bind: the RCCL library to use (NULL: "librccl.so.1"); an
 * instance the process has already loaded (e.g. PyTorch's) is reused.  cf2_xchg_unique_id: on one
 * rank, the 128-byte id every rank passes to cf2_xchg_create (collective: all ranks call it
 * together; depth 2..8 buffer regions).  cf2_xchg_register: the buffers, once: obs [n, 2 OL + 8] /
 * reset uint8 [n] per region (depth each), send (cf2_xchg_send_words, zeroed) and recv
 * (cf2_xchg_recv_words) for batches of up to kmax env-steps, age [world n], overflow, pred (the
 * look-ahead ring [npred][world], used when watch_age is on; npred >= 33).  Every publish / batch
 * takes the next region (0, 1, ..., depth - 1, 0, ...; `region` must name it: the caller keeps the
 * count) and first makes env_stream wait for the all-gather that last read that region.  A batch of
 * nb steps at capacity cap leaves recv region q as [world][nb][cf2_obs_packed_words(n, OL, cap)]:
 * the packed buffer of its step s for rank r at (r * nb + s) * words, i.e. cf2_obs_rows with
 * stride nb * words.
 * cf2_xchg_publish(x, k, cap, region, env_stream): the exchange of env-step k, whose env-step the
 * caller issued on env_stream into obs / reset of `region` (after cf2_xchg_wait_free(x, region,
 * env_stream)); packs it on env_stream, and the exchange runs inline on env_stream too.
 * cf2_xchg_run: env-steps k0 .. k0 + nb - 1 of ctx (nb <=
 * kmax; actions of step k at act_dev[k % nact]) issued back to back on env_stream with their pack
 * fused in (cf2_step_packed), then the batch's exchange at
 * capacity cap; pred_host (pinned, npred x world words, or NULL) receives the look-ahead ring after
 * the batch's consume; the batch's exchange runs on the library's exchange stream (forked from
 * env_stream), so the next batch's env-steps overlap it.  cf2_xchg_env_step: one env-step and its
 * exchange inline on env_stream (no fork, no event: for a consumer that needs every step's rows
 * before it issues the next step; pred_host as for cf2_xchg_run).  Callers on other streams are
 * ordered after inline exchanges by cf2_xchg_wait / wait_free / the next region take.  The same batch with its
 * actions given one env-step at a time (a policy in the loop, acting on each step's local rows):
 * cf2_xchg_begin(x, cap, region, env_stream) opens it (takes the region), cf2_xchg_step(x, ctx, act,
 * rew, trunc, cost, level, env_stream) issues its next env-step (up to kmax), cf2_xchg_end(x, k0,
 * pred_host, env_stream) issues its exchange; cf2_xchg_run is begin + nb steps + end.  cf2_xchg_wait(x, stream): a
 * stream waits until every exchange issued so far is complete.  cf2_xchg_pred_to_host(x, pred_host,
 * stream): the same wait, then the look-ahead ring to pred_host.  Both ring copies are device stores
 * into the pinned buffer's mapping (a kernel on the stream), which never hold the calling thread;
 * memory that is not mapped pinned memory falls back to hipMemcpyAsync.  RCCL failures return
 * CF2_ERR_HIP. */
typedef struct cf2_xchg cf2_xchg;
int  cf2_xchg_bind(const char* rccl_path);
int  cf2_xchg_unique_id(uint8_t* id_out, size_t id_len);
int  cf2_xchg_create(const uint8_t* id, size_t id_len, uint32_t world, uint32_t rank, uint32_t depth,
                     cf2_xchg** out);
int  cf2_xchg_destroy(cf2_xchg* x);
size_t cf2_xchg_send_words(uint32_t n, uint32_t obs_len, uint32_t depth, uint32_t kmax);
size_t cf2_xchg_recv_words(uint32_t n, uint32_t obs_len, uint32_t world, uint32_t depth, uint32_t kmax);
int  cf2_xchg_register(cf2_xchg* x, uint32_t n, uint32_t obs_len, uint32_t watch_age, uint32_t kmax,
                       float* const* obs_dev, uint8_t* const* reset_dev, uint32_t* send_dev, uint32_t* recv_dev,
                       uint16_t* age_dev, uint32_t* overflow_dev, uint32_t* pred_dev, uint32_t npred);
int  cf2_xchg_publish(cf2_xchg* x, uint64_t k, uint32_t cap, uint32_t region, void* env_stream);
int  cf2_xchg_wait_free(cf2_xchg* x, uint32_t region, void* stream);
int  cf2_xchg_wait(cf2_xchg* x, void* stream);
int  cf2_xchg_pred_to_host(cf2_xchg* x, uint32_t* pred_host, void* stream);
int  cf2_xchg_run(cf2_xchg* x, cf2_ctx* ctx, uint64_t k0, uint32_t nb, uint32_t cap, uint32_t region,
                  const float* const* act_dev, uint32_t nact, float* rew_dev, uint8_t* trunc_dev, float* cost_dev,
                  float* level_dev, uint32_t* pred_host, void* env_stream);
int  cf2_xchg_begin(cf2_xchg* x, uint32_t cap, uint32_t region, void* env_stream);
int  cf2_xchg_step(cf2_xchg* x, cf2_ctx* ctx, const float* act_dev, float* rew_dev, uint8_t* trunc_dev, float* cost_dev,
                   float* level_dev, void* env_stream);
int  cf2_xchg_end(cf2_xchg* x, uint64_t k0, uint32_t* pred_host, void* env_stream);
int  cf2_xchg_env_step(cf2_xchg* x, cf2_ctx* ctx, uint64_t k, uint32_t cap, uint32_t region, const float* act_dev,
                       float* rew_dev, uint8_t* trunc_dev, float* cost_dev, float* level_dev, uint32_t* pred_host,
                       void* env_stream);
/* cf2_xchg_copy_sync: the host waits for the latest look-ahead count copy into pred_host (a buffer
 * an exchange of cf2_xchg_run / cf2_xchg_end was given; up to 64 distinct buffers per exchange);
 * CF2_ERR_INVALID_ARG for a buffer no exchange copied into. */
int  cf2_xchg_copy_sync(cf2_xchg* x, const uint32_t* pred_host);
/* Diagnostics (no reference counterpart): host time of the exchange's C calls by part, ns summed
 * over the cf2_xchg_run / cf2_xchg_env_step calls counted in *calls_out -- [0] whole calls, [1] the
 * region take, [2] env-step launches, [3] the fork to the exchange stream, [4] ncclAllGather, [5]
 * consume launches, [6] closing events and count copy (n_out >= 7).  Recorded only when
 * CF2_XCHG_HOST_TIMING=1 was set at cf2_xchg_create; reset != 0 clears them. */
int  cf2_xchg_host_times(cf2_xchg* x, double* ns_out, uint32_t n_out, uint64_t* calls_out, int reset);

/* HJ value-table generation (no reference counterpart in its repository: the reference's tables come
 * from a solver that is not part of it, so parity with those tables is unpinned).  A backward
 * reachability solve of the attitude / body-rate model
 *   x = [roll phi, pitch theta, yaw psi, p, q, r]   (the C-order axes of a value table)
 *   f0 = p + (q sin(phi) + r cos(phi)) tan(theta)     f3 = c3 q r + (u0 + d0) / Ixx   c3 = (Iyy - Izz) / Ixx
 *   f1 = q cos(phi) - r sin(phi)                      f4 = c4 p r + (u1 + d1) / Iyy   c4 = (Izz - Ixx) / Iyy
 *   f2 = (q sin(phi) + r cos(phi)) / cos(theta)       f5 = c5 p q + (u2 + d2) / Izz   c5 = (Ixx - Iyy) / Izz
 *   |u_i| <= umax[i], |d_i| <= dmax[i]
 * on the grid of n[0] x ... x n[5] nodes grid_min[d] + k dx[d] (bit d of periodic_mask: dimension d
 * wraps, its upper end excluded).  u_max_player / d_max_player != 0: that input maximises the
 * Hamiltonian, else it minimises.  The scheme (first-order per-node Lax-Friedrichs, forward Euler,
 * fp64) is stated at the head of csrc/cf2sim_hjsolve.hip.
 * cf2_hj_time_step (host only): dt = cfl / max over nodes of sum_d alpha_d(x) / dx[d], the scheme's
 * monotonicity bound (alpha_d = |f_d| for d < 3, |c_d (product of the other rates)| + (umax + dmax) / I
 * for d >= 3).
 * cf2_hj_solve: steps - 1 steps of dt and one of dt_last from W = w_dev (the target function l, n[0] x
 * ... x n[5] doubles in C order) by W_t = min(0, H) (tube != 0: a backward reachable tube) or W_t = H;
 * the result ends in w_dev, tmp_dev (as large) is scratch.  table_out_dev (optional): W rounded to
 * float32, the layout cf2_bind_hj_tables takes.  change_dev (optional, one double): max |W' - W| of
 * the last step.  Asynchronous on the stream: a fixed sequence of launches, no host read.
 * CF2_ERR_INVALID_ARG, before the device is touched, for null or aliased buffers, an n[d] < 3, 2^31 or
 * more nodes, a dt, dx or inertia that is not positive, a negative umax or dmax; CF2_ERR_UNSUPPORTED for
 * an n[d] above 48. */
typedef struct cf2_hj_model {
    uint32_t n[6];
    double grid_min[6], dx[6];
    uint32_t periodic_mask;
    double inertia[3], umax[3], dmax[3];
    int32_t u_max_player, d_max_player;
} cf2_hj_model;
size_t cf2_hj_model_sizeof(void);
int  cf2_hj_time_step(const cf2_hj_model* model, double cfl, double* dt_out);
int  cf2_hj_solve(const cf2_hj_model* model, double* w_dev, double* tmp_dev, uint32_t steps, double dt,
                  double dt_last, int tube, float* table_out_dev, double* change_dev, void* stream);

/* Measurement support (no reference counterpart): streaming kernels over `bytes` (a multiple of
 * 16, both pointers 16-B aligned) with non-temporal accesses.  mode 0: copy src -> dst; mode 1:
 * read src only (bytes >= 4096; dst must hold 4 KB and is normally left untouched).  bench.py times
 * them on 2 GiB to measure the box's HBM rates. */
int  cf2_hbm_probe(void* dst_dev, const void* src_dev, size_t bytes, int mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CF2SIM_H */
