"""The large-N env kernels (step_kernel / reset paths above 32 768 envs, 256 envs per block) against
the fp32 CPU restatement (oracle/), per compiled instance and at ragged env counts.

Every instance that CF2_DISPATCH compiles (noise x DR x {Bullet SPEC 1, Bullet SPEC 2, Bullet
generic, Simple generic} = 16) runs at the smallest env counts that select the large kernels and
leave a partial last block: N1 = 33 089 (65 envs in the last block: one full wave plus one lane),
N4 = 33 092 for the 4-drone formations (68 envs) and N0 = 32 769 (a single env).  Three slices of
each launch are compared with an OracleEnv of the slice alone (env_id_offset = slice start): the
start, one straddling a block boundary, and the tail (the last full block plus the partial one).

Resynchronised loop, no env exempt: before every env-step the restatement's slices are loaded with
the kernel's own state, both sides step, and the outputs AND the state after the step are compared
before the next resynchronisation (a state sector the kernel stored wrongly would otherwise be
loaded into the restatement too).  Bounds, the project's own:
  * observation and final_obs rows 2e-5 mixed abs/rel, reward 1e-5 relative to 1 + |r|;
  * done, truncated, disturbance_level and cost exact; every integer state row exact;
  * float state 2e-5 (the one-step band: in the noise-free layout those fields are the observation).
    A field that no observation carries may take 4 x the one-step difference between the f32 and
    the f64 restatement started from the same state, where that exceeds 2e-5.  Measured on the CPU
    over every case of this file (tail slices, all env-steps, envs whose done flag agrees), the
    largest per field group: motor_lo 6.0e-8, abuf 5.6e-8, params 2.1e-8, bias 2.9e-9, dstb 6.9e-10,
    level 0, held 2.5e-7, rpy 5.7e-7; for comparison the fields an observation carries: core
    3.9e-6, obs_prev 8.3e-6, lpf 8.3e-6 (the filtered rates are the observation's), motor 5.8e-8,
    ou 1.6e-8.  4 x any of the first group stays far below 2e-5, so no field gets a wider band:
    every compared field is held to 2e-5.  Only fields that the configuration's kernels keep are
    compared (parity_util.state_fields); the others are exported as zero or stale.
Asserted on the restatement's own done flags: every case auto-resets envs of the partial last
block; the max_episode_steps=7 cases reset all of its 65 envs in one step (two full reset chunks
of 32 plus one env); every other case has a step that resets some but not all of them (in the
max_episode_steps=7 cases no env crashes within 7 env-steps, so their resets stay in lockstep).

The second half edits the parameters that the large kernels re-read from the kernarg segment
(late_epilogue, late_sensor, late_reset) off their defaults, several of which are zero, and runs
the same loop above and below the kernel threshold.
"""
import numpy as np
import pytest
import torch

import oracle as O
from cf2sim.config import build_config
from parity_util import (ALL_DISPATCH_KEYS, LISTED_GROUPS, N0, N1, N4, copy_config, dispatch_key, edit_cost, edit_done,
                         edit_reset, edit_reward, edit_sensor, large_slices, nerr, partial_block, state_fields,
                         wide_actions)

FREE, HOVER, SIMPLE = ("DroneHoverBulletFreeEnvWithoutAdversary-v0", "DroneHoverBulletEnv-v0",
                       "DroneHoverSimpleEnv-v0")
GUST, DOWNWASH = "DroneHoverBulletFreeEnvWithGust-v0", "DroneHoverBulletFreeEnvWithDownwash-v0"
NO_NOISE, NO_DR = dict(observation_noise=0), dict(domain_randomization=0)
CLEAN = dict(observation_noise=0, domain_randomization=-1, motor_thrust_noise=0)
SEED = 3
gpu_test = pytest.mark.gpu

# label -> (env id, env count, env-steps, kwargs); one or more per compiled instance
CASES = {
    # <noise, DR, Bullet, SPEC 1>: the reference-default shape, single drones
    "s1-n1d1-gust": (GUST, N1, 40, {}),
    "s1-n1d1-gust-n0": (GUST, N0, 40, {}),
    "s1-n0d0-clean": (FREE, N1, 40, CLEAN),
    "s1-n0d1-hover": (HOVER, N1, 40, NO_NOISE),                        # the hover-task reward
    "s1-n1d0-t7": (FREE, N1, 40, dict(max_episode_steps=7, **NO_DR)),
    # <., ., Bullet, SPEC 0>: the generic shape
    "s0-n1d1-agg1": (FREE, N1, 60, dict(aggregate_phy_steps=1)),        # held obs persists
    "s0-n1d1-ring4": (FREE, N1, 40, dict(latency=0.02)),                # latency ring of 4
    "s0-n1d1-nolat-t7": (FREE, N1, 40, dict(latency=0.0, max_episode_steps=7)),
    "s0-n0d0-ring4": (FREE, N1, 40, dict(latency=0.02, **CLEAN)),
    "s0-n0d1-agg1": (FREE, N1, 60, dict(aggregate_phy_steps=1, **NO_NOISE)),
    "s0-n1d0-nolat-t7": (FREE, N1, 40, dict(latency=0.0, max_episode_steps=7, **NO_DR)),
    # <., ., Simple, SPEC 0>
    "simple-n1d1": (SIMPLE, N1, 40, {}),
    "simple-n0d1": (SIMPLE, N1, 40, NO_NOISE),
    "simple-n1d0": (SIMPLE, N1, 40, NO_DR),
    "simple-n0d0": (SIMPLE, N1, 40, CLEAN),
    # <., ., Bullet, SPEC 2>: 4-drone formations with downwash, the horizon of test_gpu_parity's f4
    "s2-n1d1": (DOWNWASH, N4, 25, {}),
    "s2-n0d1": (DOWNWASH, N4, 25, NO_NOISE),
    "s2-n1d0": (DOWNWASH, N4, 25, NO_DR),
    "s2-n0d0": (DOWNWASH, N4, 25, CLEAN),
}
FREE_RUNNING = ("s1-n0d0-clean", "simple-n1d1", "s0-n1d1-ring4")


def test_cases_cover_every_compiled_instance():
    """The CF2_DISPATCH key of every case, recomputed from its CF2Config (noise on, DR on, physics,
    default shape, num_drones): the cases cover all 16 compiled instances, and every env count
    selects the large kernels."""
    keys = {}
    for label, (env_id, n, T, kw) in CASES.items():
        keys.setdefault(dispatch_key(build_config(env_id, n, seed=SEED, **kw)), []).append(label)
        assert n > 32768
    assert len(ALL_DISPATCH_KEYS) == 16
    assert set(keys) == ALL_DISPATCH_KEYS, sorted(ALL_DISPATCH_KEYS - set(keys))
    assert dispatch_key(build_config(GUST, N0, seed=SEED)) == (1, 1, "B", 1)
    for n, last in ((N1, 65), (N4, 68), (N0, 1)):
        lo, hi = partial_block(n)
        assert hi - lo == last and lo % 256 == 0
        assert large_slices(n)[-1] == (lo - 256, n)
    assert N4 % 4 == 0 and all(lo % 4 == 0 for lo, _ in large_slices(N4))


class _Pair:
    """The kernel on all n envs and the fp32 restatement on slices of them."""

    def __init__(self, env_id, cfg, slices):
        from cf2sim.vec_env import BatchedCrazyflieEnv
        self.n = int(cfg.num_envs)
        self.cfg = cfg
        self.slices = slices
        self.env = BatchedCrazyflieEnv(env_id, self.n, config=copy_config(cfg), want_final_obs=True)
        self.refs = [O.OracleEnv(copy_config(cfg, num_envs=hi - lo, env_id_offset=int(cfg.env_id_offset) + lo), "f32")
                     for lo, hi in slices]
        self.groups = state_fields(cfg)
        self.fig = dict(obs=0.0, rew=0.0, state=0.0, state_group="", resets=0)

    def state(self):
        sf, si = self.env.get_state()
        return sf.cpu().numpy(), si.cpu().numpy()

    def load(self, gsf, gsi):
        for (lo, hi), r in zip(self.slices, self.refs):
            r.set_state(np.ascontiguousarray(gsf[:, lo:hi]), np.ascontiguousarray(gsi[:, lo:hi]))

    def reset(self):
        go = self.env.reset().cpu().numpy()
        for (lo, hi), r in zip(self.slices, self.refs):
            self.fig["obs"] = max(self.fig["obs"], nerr(go[lo:hi], r.reset()))

    def step(self, a, t):
        """One env-step of both sides: the exact outputs asserted, the float errors accumulated.
        Returns the restatement's done flags per slice."""
        g_o, g_r, g_d, g_i = self.env.step(torch.from_numpy(a).cuda())
        g_o, g_r, g_d = g_o.cpu().numpy(), g_r.cpu().numpy(), g_d.cpu().numpy().astype(bool)
        g_t, g_c = g_i["truncated"].cpu().numpy().astype(bool), g_i["cost"].cpu().numpy()
        g_l, g_f = g_i["disturbance_level"].cpu().numpy(), g_i["final_obs"].cpu().numpy()
        dones = []
        for (lo, hi), r in zip(self.slices, self.refs):
            r_o, r_r, r_d, r_i = r.step(a[lo:hi], want_final=True)
            where = f"env-step {t}, envs [{lo}, {hi})"
            np.testing.assert_array_equal(g_d[lo:hi], r_d, err_msg="done, " + where)
            np.testing.assert_array_equal(g_t[lo:hi], r_i["truncated"], err_msg="truncated, " + where)
            np.testing.assert_array_equal(g_c[lo:hi], r_i["cost"].astype(np.float32), err_msg="cost, " + where)
            np.testing.assert_array_equal(g_l[lo:hi], r_i["level"].astype(np.float32), err_msg="level, " + where)
            self.fig["obs"] = max(self.fig["obs"], nerr(g_o[lo:hi], r_o))
            self.fig["rew"] = max(self.fig["rew"], nerr(g_r[lo:hi], r_r))
            if self.cfg.auto_reset and r_d.any():
                self.fig["obs"] = max(self.fig["obs"], nerr(g_f[lo:hi][r_d], r_i["final_obs"][r_d]))
            self.fig["resets"] += int(r_d.sum())
            dones.append(r_d)
        self.costs = [g_c[lo:hi] for lo, hi in self.slices]
        return dones

    def compare_state(self, gsf, gsi, t, int_rows=range(5), groups=None):
        for (lo, hi), r in zip(self.slices, self.refs):
            rsf, rsi = r.get_state()
            for row in int_rows:
                np.testing.assert_array_equal(gsi[row, lo:hi], rsi[row], err_msg=f"int state row {row}, env-step {t}, "
                                                                                f"envs [{lo}, {hi})")
            for name, f in self.groups.items():
                if groups is not None and name not in groups:
                    continue
                e = nerr(gsf[f, lo:hi], rsf[f])
                if e > self.fig["state"]:
                    self.fig["state"], self.fig["state_group"] = e, f"{name} (env-step {t}, envs [{lo}, {hi}))"

    def close(self):
        self.env.check_device_errors()
        self.env.close()
        for r in self.refs:
            r.close()


class _PartialBlock:
    """Auto-resets inside the partial last block, counted on the restatement's done flags."""

    def __init__(self, n, slices):
        lo, hi = partial_block(n)
        self.off = lo - slices[-1][0]
        self.size = hi - lo
        self.per_step = []

    def add(self, tail_done):
        self.per_step.append(int(tail_done[self.off:].sum()))

    def check(self, label, all_at_once):
        total = sum(self.per_step)
        print(f"{label}: resets in the partial block of {self.size} envs: {total} over {len(self.per_step)} env-steps, "
              f"largest in one step {max(self.per_step)}")
        assert total > 0, "no auto-reset in the partial last block"
        if all_at_once:       # two full reset chunks of 32 plus a partial one, in a partial block
            assert max(self.per_step) == self.size
        elif self.size > 1:
            assert any(0 < k < self.size for k in self.per_step), "no step resets some but not all of the block"


def _report(label, fig):
    print(f"{label}: worst obs {fig['obs']:.3g}, reward {fig['rew']:.3g}, state {fig['state']:.3g} "
          f"[{fig['state_group']}], resets in the slices {fig['resets']}")


def _resynchronised(label, env_id, cfg, T, slices, partial=True, all_at_once=False):
    n = int(cfg.num_envs)
    p = _Pair(env_id, cfg, slices)
    pb = _PartialBlock(n, slices)
    p.reset()
    rng = np.random.default_rng(5)
    gsf, gsi = p.state()
    costs = []
    for t in range(T):
        p.load(gsf, gsi)
        dones = p.step(wide_actions(rng, n), t)
        pb.add(dones[-1])
        costs.extend(p.costs)
        gsf, gsi = p.state()
        p.compare_state(gsf, gsi, t)
    p.close()
    _report(label, p.fig)
    assert p.fig["obs"] < 2e-5 and p.fig["rew"] < 1e-5 and p.fig["state"] < 2e-5, p.fig
    if partial:
        pb.check(label, all_at_once)
    assert p.fig["resets"] > 0
    return p.fig, np.concatenate(costs)


@gpu_test
@pytest.mark.parametrize("label", list(CASES))
def test_large_kernel_instance_matches_restatement_resynchronised(gpu, label):
    env_id, n, T, kw = CASES[label]
    cfg = build_config(env_id, n, seed=SEED, **kw)
    _resynchronised(label, env_id, cfg, T, large_slices(n), all_at_once=kw.get("max_episode_steps") == 7)


@gpu_test
@pytest.mark.parametrize("label", FREE_RUNNING)
def test_large_kernel_instance_matches_restatement_free_running(gpu, label):
    """Without resynchronisation, over the same env-steps, in the band of
    test_kernel_matches_fp32_restatement: 5e-4 on observations and on the state fields it lists,
    done exact at every step, episode and RNG counters exact at the end."""
    env_id, n, T, kw = CASES[label]
    cfg = build_config(env_id, n, seed=SEED, **kw)
    p = _Pair(env_id, cfg, large_slices(n))
    p.reset()
    assert p.fig["obs"] < 2e-5, p.fig
    rng = np.random.default_rng(5)
    for t in range(T):
        p.step(wide_actions(rng, n), t)
    gsf, gsi = p.state()
    p.compare_state(gsf, gsi, T - 1, int_rows=(0, 1), groups=LISTED_GROUPS)
    p.close()
    _report(label + " free-running", p.fig)
    assert p.fig["obs"] < 5e-4 and p.fig["state"] < 5e-4, p.fig
    assert p.fig["resets"] > 0


@gpu_test
def test_large_kernel_without_auto_reset(gpu):
    """auto_reset off and no TimeLimit: the epilogue's branch without resets.  Finished envs stay
    as they are and keep stepping; their outputs and state are compared like every other env's."""
    label = "no-auto-reset"
    cfg = build_config(GUST, N1, seed=SEED, auto_reset=False, max_episode_steps=0)
    slices = large_slices(N1)
    fig, _ = _resynchronised(label, GUST, cfg, 40, slices, partial=False)


@gpu_test
def test_large_kernel_masked_reset(gpu):
    """reset(mask) at N1 after a few env-steps, the mask covering part of the partial last block:
    the reset observations and the whole state of the slices equal ref.reset(mask)."""
    cfg = build_config(GUST, N1, seed=SEED)
    slices = large_slices(N1)
    p = _Pair(GUST, cfg, slices)
    p.reset()
    rng = np.random.default_rng(5)
    for t in range(5):
        p.load(*p.state())
        p.step(wide_actions(rng, N1), t)
    gsf, gsi = p.state()
    p.load(gsf, gsi)
    mask = (np.arange(N1) % 3 == 0).astype(np.uint8)
    lo, hi = partial_block(N1)
    assert 0 < mask[lo:hi].sum() < hi - lo
    go = p.env.reset(torch.from_numpy(mask).cuda()).cpu().numpy()
    worst = 0.0
    for (lo, hi), r in zip(slices, p.refs):
        m = mask[lo:hi].astype(bool)
        worst = max(worst, nerr(go[lo:hi][m], r.reset(mask[lo:hi])[m]))
    gsf, gsi = p.state()
    p.compare_state(gsf, gsi, 5)
    p.close()
    print(f"masked reset: worst obs {worst:.3g}, state {p.fig['state']:.3g} [{p.fig['state_group']}]")
    assert worst < 2e-5 and p.fig["state"] < 2e-5, (worst, p.fig)


# ---- parameters that reach the large kernel through the late re-reads ----
def _reset_fixed(c):
    c.enable_reset_distribution = 0
    return edit_reset(c)


EDITS = {"reward": edit_reward, "cost": edit_cost, "done": edit_done, "reset": edit_reset,
         "reset-no-distribution": _reset_fixed, "sensor": edit_sensor}


@gpu_test
@pytest.mark.parametrize("n", [N1, 300])
@pytest.mark.parametrize("edit", list(EDITS))
def test_edited_parameters_match_restatement(gpu, edit, n):
    """A CF2Config built by build_config, edited, and given to the kernel and to the restatement:
    at N1 the large kernel reads the edited fields through late_epilogue / late_sensor /
    late_reset, at 300 envs the small kernel reads them from its plain parameter block."""
    cfg = EDITS[edit](build_config(GUST, n, seed=SEED))
    large = n > 32768
    fig, cost = _resynchronised(f"edit-{edit}-{n}", GUST, cfg, 40, large_slices(n) if large else [(0, n)], partial=large)
    if edit == "cost":
        zero = float((cost == 0.0).mean())
        print(f"edit-cost-{n}: share of cost 0: {zero:.3f}")
        assert set(np.unique(cost)) == {0.0, 1.0} and 0.1 <= zero <= 0.9, zero
