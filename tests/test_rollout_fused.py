"""cf2_rollout: K env-steps fused in one launch (state in registers) must equal K cf2_step calls
with the same actions -- observations, rewards, dones, truncations, costs, levels, final
observations and the state afterwards -- across auto-resets, TimeLimit truncations, the noise /
DR / gust / HJ / formation paths and launches that the host splits into residency slices."""
import numpy as np
import pytest
import torch

from cf2sim.config import build_config
from parity_util import N1, N4, edit_done, edit_physics, edit_reset, edit_reward

pytestmark = pytest.mark.gpu

CASES = [
    ("DroneHoverBulletFreeEnvWithGust-v0", 3000, {}),
    ("DroneHoverBulletFreeEnvWithoutAdversary-v0", 1024, dict(max_episode_steps=7)),
    ("DroneHoverSimpleEnv-v0", 777, {}),
    ("DroneHoverBulletFreeEnvWithConstWind-v0", 512, dict(observation_noise=0)),
    ("DroneHoverBulletFreeEnvWithDownwash-v0", 1024, {}),
    ("DroneHoverBulletFreeEnvWithoutAdversary-v0", 512, dict(aggregate_phy_steps=1, latency=0.02, max_episode_steps=9)),
    ("DroneHoverBulletFreeEnvWithGust-v0", 150000, {}),       # > one residency round: sliced
]
FREE = "DroneHoverBulletFreeEnvWithoutAdversary-v0"
# rollout_kernel (above 32 768 envs) with a partial last block and wave, on the instances other
# than the noisy, domain-randomised default: N1 = 33 089 envs, N4 = 33 092 for the formations
LARGE_CASES = [
    (FREE, N1, dict(observation_noise=0, domain_randomization=-1, motor_thrust_noise=0)),
    ("DroneHoverSimpleEnv-v0", N1, dict(max_episode_steps=7)),
    (FREE, N1, dict(aggregate_phy_steps=1)),
    (FREE, N1, dict(latency=0.02, max_episode_steps=7)),
    ("DroneHoverBulletFreeEnvWithDownwash-v0", N4, {}),
]


@pytest.mark.parametrize("env_id,n,kw", CASES)
def test_fused_rollout_equals_step_loop(gpu, env_id, n, kw):
    _compare(gpu, env_id, n, kw)


@pytest.mark.parametrize("env_id,n,kw", LARGE_CASES)
def test_fused_rollout_equals_step_loop_large_ragged(gpu, env_id, n, kw):
    _compare(gpu, env_id, n, kw)


def _edited_epilogue(c):
    return edit_reset(edit_done(edit_reward(c)))


@pytest.mark.parametrize("env_id,kw,edit", [
    ("DroneHoverBulletFreeEnvWithGust-v0", {}, _edited_epilogue),       # late_epilogue, late_reset
    (FREE, dict(domain_randomization=0), edit_physics),                 # late_physics, late_io
])
def test_fused_rollout_with_edited_parameters(gpu, env_id, kw, edit):
    """Reward weights and targets, done limits, reset limits and (DR off) the physics constants
    off their defaults: the fused rollout re-reads them from the kernarg segment (LATEX)."""
    _compare(gpu, env_id, N1, {}, config=edit(build_config(env_id, N1, seed=9, **kw)))


@pytest.mark.parametrize("n", [2000, 40000])
def test_fused_rollout_boltzmann_hj_levels(gpu, n):
    """The Boltzmann-level HJ env: a reset redraws the episode's level, which the small-N
    rollout's helper waves track from step to step for their speculative resets."""
    from test_gpu_parity import _synthetic_tables
    V = torch.from_numpy(_synthetic_tables(tuple(range(3)), seed=1)).cuda()
    tol = [lv % 3 for lv in range(21)]
    _compare(gpu, "DroneHoverBulletFreeEnvWithRandomHJAdversary-v0", n, dict(max_episode_steps=6),
             setup=lambda e: e.bind_hj_tables(V, tol))


def _compare(gpu, env_id, n, kw, setup=None, config=None):
    """config: a ready CF2Config (for n envs) that both envs get instead of build_config's."""
    from cf2sim.vec_env import BatchedCrazyflieEnv
    from parity_util import copy_config
    K = 24
    if config is not None:
        kw = dict(config=copy_config(config))
    a = (torch.rand(K, n, 4, device=gpu, generator=torch.Generator(device=gpu).manual_seed(3)) * 2 - 1).contiguous()
    ref = BatchedCrazyflieEnv(env_id, n, seed=9, want_final_obs=True, **kw)
    fus = BatchedCrazyflieEnv(env_id, n, seed=9, want_final_obs=True, **kw)
    if setup is not None:
        setup(ref)
        setup(fus)
    ref.reset()
    fus.reset()
    outs = {k: [] for k in ("obs", "rew", "done", "trunc", "cost", "level", "fin")}
    for k in range(K):
        o, r, d, info = ref.step(a[k])
        for key, t in (("obs", o), ("rew", r), ("done", d), ("trunc", info["truncated"]), ("cost", info["cost"]),
                       ("level", info["disturbance_level"]), ("fin", info["final_obs"])):
            outs[key].append(t.clone())
    o, r, d, info = fus.rollout(a)
    done = torch.stack(outs["done"]).bool()
    assert done.any(), "no auto-reset inside the window"
    torch.testing.assert_close(d, torch.stack(outs["done"]), rtol=0, atol=0)
    torch.testing.assert_close(info["truncated"], torch.stack(outs["trunc"]), rtol=0, atol=0)
    for key, got in (("obs", o), ("rew", r), ("cost", info["cost"]), ("level", info["disturbance_level"])):
        torch.testing.assert_close(got, torch.stack(outs[key]), rtol=1e-6, atol=1e-6, msg=key)
    fin = info["final_obs"][done]
    torch.testing.assert_close(fin, torch.stack(outs["fin"])[done], rtol=1e-6, atol=1e-6)
    gs, gi = fus.get_state()
    rs, ri = ref.get_state()
    torch.testing.assert_close(gi, ri, rtol=0, atol=0)
    torch.testing.assert_close(gs, rs, rtol=1e-6, atol=1e-6)
    # continuing with single steps from the rollout's final state stays identical
    b = torch.rand(n, 4, device=gpu) * 2 - 1
    o1 = ref.step(b)[0].clone()
    o2 = fus.step(b)[0]
    torch.testing.assert_close(o2, o1, rtol=1e-6, atol=1e-6)
    ref.close()
    fus.close()


def test_rollout_rejects_bad_buffers(gpu):
    from cf2sim.vec_env import BatchedCrazyflieEnv
    env = BatchedCrazyflieEnv("DroneHoverBulletFreeEnvWithoutAdversary-v0", 64)
    env.reset()
    with pytest.raises(ValueError):
        env.rollout(torch.zeros(4, 63, 4, device=gpu))
    with pytest.raises(ValueError):
        env.rollout(torch.zeros(4, 64, 4, device=gpu, dtype=torch.float64))
    env.close()
