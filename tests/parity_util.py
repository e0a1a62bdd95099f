"""Shared helpers of the parity tests: the closed-loop test controller and the state error
metric of BASELINE.json's "state within 1e-4 rel over 240 steps"."""
import numpy as np

CLEAN = dict(observation_noise=0, domain_randomization=-1, motor_thrust_noise=0, max_episode_steps=0)


def pd_actions(state17, hover, kp=0.5, kd=0.08, kz=0.05):
    """A stabilising attitude/altitude PD controller on obs17 = [p, q, v, w_body, a] (test helper;
    stands in for a trained policy closing the loop on the env's own observations).  kp / kd: roll
    and pitch angle / rate gains, kz: yaw-rate gain."""
    p, q, v, w = state17[:, 0:3], state17[:, 3:7], state17[:, 7:10], state17[:, 10:13]
    x, y, z, qw = q.T
    roll = np.arctan2(2 * (qw * x + y * z), 1 - 2 * (x * x + y * y))
    pitch = np.arcsin(np.clip(2 * (qw * y - z * x), -1, 1))
    T = hover + 0.5 * (1.0 - p[:, 2]) - 0.4 * v[:, 2]
    tx, ty, tz = -kp * roll - kd * w[:, 0], -kp * pitch - kd * w[:, 1], -kz * w[:, 2]
    a = (T[:, None] + tx[:, None] * np.array([-1, -1, 1, 1]) + ty[:, None] * np.array([-1, 1, 1, -1])
         + tz[:, None] * np.array([-1, 1, -1, 1]))
    return np.clip(a, -1, 1).astype(np.float32)


STATE_BLOCKS = {"pos": slice(0, 3), "quat": slice(3, 7), "vel": slice(7, 10), "omega": slice(10, 13)}


def state_rel_err(g, r):
    """Relative state error of BASELINE.json's "state within 1e-4 rel over 240 steps", per env and
    per state vector (position, quaternion, linear velocity, angular velocity):
    ||g - r||_2 / max(||r||_2, 1).  Norm-wise because a component-wise ratio is not invariant
    under a rotation of the world frame (the error of a spinning drone leaks between components);
    the floor of 1 (m, unit quaternion, m/s, rad/s) only acts on velocity vectors near hover, where
    a pure ratio is undefined.  Returns {block: [N] errors}."""
    return {k: np.linalg.norm(g[b] - r[b], axis=0) / np.maximum(np.linalg.norm(r[b], axis=0), 1.0)
            for k, b in STATE_BLOCKS.items()}


# ---- the large-N env kernels (above SMALL_N_MAX = 32 768 envs: 256 envs per block) ----
SMALL_N_MAX = 32768
N1 = SMALL_N_MAX + 256 + 65     # single drones: the last block holds 65 envs, one full wave plus one lane
N4 = 33092                      # 4-drone formations: a multiple of 4, the last block holds 68 envs
N0 = SMALL_N_MAX + 1            # the last block holds a single env
SLICE = 512


def nerr(g, r):
    """Mixed abs/rel error |g - r| / (1 + |r|), the suite's metric."""
    return float((np.abs(g - r) / (1.0 + np.abs(r))).max()) if np.size(g) else 0.0


def wide_actions(rng, n):
    """The ragged-count test's actions: wide enough that envs crash and auto-reset within tens of steps."""
    return (rng.uniform(-1, 1, size=(n, 4)) * 0.6 + 0.1111).astype(np.float32)


def copy_config(cfg, **fields):
    """A copy of a CF2Config with some fields replaced (scalars only)."""
    c = type(cfg).from_buffer_copy(bytes(cfg))
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def large_slices(n):
    """The slices of a large launch compared with the restatement: the start, one straddling a
    block boundary in the middle, and the tail: the last full block plus the partial one."""
    last_full = ((n - 1) // 256 - 1) * 256
    return [(0, SLICE), (16128, 16128 + SLICE), (last_full, n)]


def partial_block(n):
    """Env range of the partial last block of a 256-env-per-block launch."""
    return ((n - 1) // 256) * 256, n


def dispatch_key(cfg):
    """The kernel instance a configuration runs (csrc/cf2sim_kernels.hip, CF2_DISPATCH):
    (noise, DR, physics, SPEC), SPEC 1 = the reference-default Bullet shape with single drones,
    SPEC 2 = that shape in formations, SPEC 0 = the generic shape."""
    default_shape = (cfg.physics == 0 and cfg.aggregate_phy_steps == 2 and cfg.obs_rate == 2 and cfg.buf_size == 2
                     and bool(cfg.use_latency) and bool(cfg.use_motor_dynamics))
    spec = 0 if not default_shape else (1 if cfg.num_drones == 1 else 2)
    return (int(bool(cfg.observation_noise_on)), int(bool(cfg.domain_randomization_on)), "BS"[cfg.physics], spec)


ALL_DISPATCH_KEYS = ({(n, d, "B", s) for n in (0, 1) for d in (0, 1) for s in (0, 1, 2)}
                     | {(n, d, "S", 0) for n in (0, 1) for d in (0, 1)})

# The float fields of the public snapshot (csrc/cf2sim_internal.h, F_*) in two classes.
# LISTED: the fields test_kernel_matches_fp32_restatement compares (pose, velocities, motor and
# OU state, o_{k-1}, the action history): bounded like the observation.
# The others are only compared where the configuration's kernel keeps them (cf2sim_state.h:
# store_core / store_tail / store_env); a field the kernel does not keep is exported as stale
# or zero and means nothing.
def state_fields(cfg):
    """{group: [field indices]} of the snapshot's float fields that the kernels of cfg keep."""
    noise, dr = bool(cfg.observation_noise_on), bool(cfg.domain_randomization_on)
    ol = 13 if noise else 17
    g = {"core": list(range(0, 13)), "motor": list(range(16, 20)), "ou": list(range(20, 24)),
         "obs_prev": list(range(56, 56 + ol)), "hist_act": list(range(73, 81)),
         "abuf": list(range(24, 24 + 4 * int(cfg.buf_size)))}
    if cfg.physics == 1:
        g["rpy"] = [13, 14, 15]
    if noise:
        g["bias"] = [40, 41, 42]
        g["lpf"] = [43, 44, 45]
        if cfg.aggregate_phy_steps % cfg.obs_rate:
            g["held"] = list(range(46, 56))
    if dr:
        g["params"] = list(range(81, 100))
    if cfg.disturbance in (3, 4):       # constant wind, gust: the episode's / current torque
        g["dstb"] = [100, 101, 102]
        g["level"] = [103]
    if cfg.level_mode == 1:             # a level drawn per episode (Boltzmann)
        g["level"] = [103]
    if cfg.use_motor_dynamics:
        g["motor_lo"] = list(range(104, 108))
    return g


LISTED_GROUPS = ("core", "motor", "ou", "obs_prev", "hist_act")


# ---- config edits: every parameter the large kernels re-read from the kernarg segment
# (late_epilogue, late_sensor, late_reset, late_physics) set off its default, pairwise different
# within its group, so that a swapped field or a wrong offset changes the result ----
def edit_reward(c):
    c.penalty_action, c.penalty_angle, c.penalty_spin, c.penalty_velocity = 0.013, 0.7, 0.31, 0.53
    c.penalty_z, c.penalty_terminal, c.penalty_arp, c.penalty_dist = 0.17, 870.0, 0.23, 0.41
    for k, v in enumerate((0.11, -0.07, 0.93)):
        c.target_pos[k] = v
    for k, v in enumerate((0.05, -0.09, 0.21)):
        c.target_rpy[k] = v
    for k, v in enumerate((0.3, -0.45, 0.15)):
        c.target_rate[k] = v
    return c


def edit_cost(c):
    c.cost_xy_lim, c.cost_z_lim, c.cost_rp_lim, c.cost_vel_lim, c.cost_rate_lim = 0.3, 1.2, 0.6, 6.0, 0.55
    return c


def edit_done(c):
    c.done_rp_limit, c.done_rate_limit_deg, c.done_z_min = 0.5, 300.0, 0.8
    return c


def edit_reset(c):
    for k, v in enumerate((0.13, -0.21, 1.17)):
        c.init_xyz[k] = v
    c.reset_pos_lim, c.reset_angle_lim, c.reset_vel_lim = 0.4, 0.35, 0.27
    c.reset_rate_lim, c.reset_yaw_rate_lim = 2.1, 0.6
    c.action_init_std, c.motor_init_std = 0.05, 0.035
    if c.domain_randomization_on:
        c.domain_randomization = 0.17
    return c


def edit_sensor(c):
    c.pos_norm_std, c.pos_unif_range, c.vel_norm_std = 0.004, 0.003, 0.023
    c.rot_norm_std, c.rot_unif_range = 0.0031, 0.0017
    c.gyro_noise_density, c.gyro_random_walk, c.gyro_turn_on_bias_sigma = 0.00041, 0.019, 0.06
    c.lpf_ratio = 0.37
    return c


def edit_physics(c):
    """DR off: the constants of the physics sub-steps (late_physics in the fused rollout)."""
    c.mass, c.drag_xy, c.drag_z, c.lin_damping = c.mass * 1.13, c.drag_xy * 1.7, c.drag_z * 0.6, 0.07
    c.motor_time_constant = 0.055
    c.B = c.time_step / c.motor_time_constant
    c.A = 1.0 - c.B
    return c
