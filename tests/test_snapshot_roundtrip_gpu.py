"""cf2_get_state -> cf2_set_state -> env-steps on the GPU, for every compiled kernel instance and
every disturbance and level mode, in the small-N and the large-N kernel family.

The protocol and the 24 cases are snapshot_util's: env A runs on, env B exports and re-imports its
own state before every env-step, env C is constructed, never reset, and imports A's state before
env-step t0.  Everything B and C return, the exported state after the last env-step and after a
masked reset are A's bit for bit (NaNs and signed zeros count): there are no tolerances.  The fp32
restatement passes the same protocol (test_snapshot_roundtrip_cpu.py), so a mismatch here belongs to
the kernels or to state_convert_kernel.

Sizes: 321 envs (five full 64-env blocks of the small-N kernels plus one lane; 324 in formations) and
parity_util.N1 = 33 089 (N4 = 33 092 in formations), the smallest counts that select each kernel
family and leave a ragged tail.

The second test reads an imported state with the fused kernels (rollout_kernel,
collect_rollout_kernel and its small variant); the third imports a snapshot whose unused o_{k-1}
entries are zero, as the restatement writes them: with sensor noise those entries lie on the gyro
low-pass slots of the internal layout, and an import must not let them reach the filter.
"""
import numpy as np
import pytest
import torch

from parity_util import N1, N4, SMALL_N_MAX, copy_config, state_fields
from snapshot_util import (CASES, FUSED_CASES, I_FLAGS, actions, check_conditions, config, hj_tables, horizon,
                           is_formation, reset_mask)
from test_action_once_gpu import _same
from test_collect_fused import _check_equal

pytestmark = pytest.mark.gpu

N_SMALL, N_SMALL_FORMATION = 321, 324
SIZES = ("small", "large")
OUTPUTS = ("obs", "rew", "done", "truncated", "cost", "disturbance_level")
_tables = {}


def _count(label, size):
    if size == "small":
        return N_SMALL_FORMATION if is_formation(label) else N_SMALL
    return N4 if is_formation(label) else N1


def _make(label, cfg):
    """A fresh env of the configuration; HJ tables are bound here: a snapshot does not carry them."""
    from cf2sim.vec_env import BatchedCrazyflieEnv
    env = BatchedCrazyflieEnv(CASES[label][0], int(cfg.num_envs), config=copy_config(cfg), want_final_obs=True)
    if cfg.disturbance == 5:
        V, tol = hj_tables()
        if "V" not in _tables:
            _tables["V"] = torch.from_numpy(V).cuda()
        env.bind_hj_tables(_tables["V"], tol[:int(cfg.num_levels)])
    return env


def _step(env, a):
    obs, rew, done, info = env.step(a)
    return dict(obs=obs, rew=rew, done=done, truncated=info["truncated"], cost=info["cost"],
                disturbance_level=info["disturbance_level"], final_obs=info["final_obs"])


def _same_outputs(got, ref, what, outputs=OUTPUTS):
    for k in outputs:
        assert _same(got[k], ref[k]), f"{what}: {k} differs"
    m = ref["done"].bool()
    assert _same(got["final_obs"][m], ref["final_obs"][m]), f"{what}: final_obs differs"


def _same_state(env, ref, groups, what):
    (gf, gi), (rf, ri) = env.get_state(), ref.get_state()
    assert _same(gi, ri), f"{what}: int rows differ"
    for name, f in groups.items():
        assert _same(gf[f], rf[f]), f"{what}: float fields of {name} differ"
    for si in (gi, ri):
        assert int((si[I_FLAGS] >> 8).max()) == 0 and int(si[I_FLAGS].min()) >= 0, \
            f"{what}: an exported flag word has bits above bit 7"


def _reimport(env):
    env.set_state(*env.get_state())


def _close(*envs):
    for e in envs:
        e.check_device_errors()
        e.close()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("label", list(CASES))
def test_snapshot_round_trip(gpu, label, size):
    n = _count(label, size)
    assert (n > SMALL_N_MAX) == (size == "large")
    cfg = config(label, n)
    T, t0 = horizon(label)
    acts = torch.from_numpy(actions(n, T)).cuda()
    groups = state_fields(cfg)
    A, B, C = _make(label, cfg), _make(label, cfg), _make(label, cfg)
    assert _same(A.reset(), B.reset())
    done = torch.zeros(T, n, dtype=torch.bool, device="cuda")
    trunc = torch.zeros(T, n, dtype=torch.bool, device="cuda")
    for t in range(T):
        if t == t0:
            sf, si = A.get_state()
            si_t0 = si.cpu().numpy()
            C.set_state(sf, si)
            # a field that no later output depends on shows here only (the held measurement where
            # aggregate_phy_steps = 1: every env-step measures anew before it emits an observation)
            _same_state(C, A, groups, "fresh env, right after the import")
        _reimport(B)
        ra = _step(A, acts[t])
        _same_outputs(_step(B, acts[t]), ra, f"re-imported env, env-step {t}")
        if t >= t0:
            _same_outputs(_step(C, acts[t]), ra, f"fresh env, env-step {t}")
        done[t], trunc[t] = ra["done"].bool(), ra["truncated"].bool()
    for env, who in ((B, "re-imported env"), (C, "fresh env")):
        _same_state(env, A, groups, f"{who}, after env-step {T - 1}")
    mask = torch.from_numpy(reset_mask(n)).cuda()
    ro = A.reset(mask)
    for env, who in ((B, "re-imported env"), (C, "fresh env")):
        assert _same(env.reset(mask)[mask], ro[mask]), f"{who}: masked reset rows differ"
        _same_state(env, A, groups, f"{who}, after the masked reset")
    _close(A, B, C)
    check_conditions(label, done.cpu().numpy(), trunc.cpu().numpy(), si_t0)


def _advance(envs, acts):
    """The same env-steps on every env; returns a copy of the last observations of the first."""
    for a in acts:
        for e in envs:
            e.step(a)
    return envs[0].obs.clone()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("label", FUSED_CASES)
def test_fused_paths_after_an_import(gpu, label, size):
    """A never-reset env that imported A's state before env-step t0 runs the next K = 8 env-steps in
    one launch: cf2_rollout on the given actions, and in a second pair the fused collect
    (cf2_collect_rollout) from the observations of env-step t0 - 1."""
    from cf2sim.rollout import FusedActorCritic, MLPActorCritic, collect
    K = 8
    n = _count(label, size)
    cfg = config(label, n)
    T, t0 = horizon(label)
    acts = torch.from_numpy(actions(n, T)).cuda()
    groups = state_fields(cfg)
    # cf2_rollout
    A, C = _make(label, cfg), _make(label, cfg)
    A.reset()
    _advance([A], acts[:t0])
    C.set_state(*A.get_state())
    window = acts[t0:t0 + K].contiguous()
    oa, ra, da, ia = A.rollout(window)
    oc, rc, dc, ic = C.rollout(window)
    assert da.any(), "no auto-reset inside the fused window"
    ref = dict(obs=oa, rew=ra, done=da, final_obs=ia["final_obs"], **{k: ia[k] for k in OUTPUTS[3:]})
    got = dict(obs=oc, rew=rc, done=dc, final_obs=ic["final_obs"], **{k: ic[k] for k in OUTPUTS[3:]})
    _same_outputs(got, ref, "rollout after the import")
    _same_state(C, A, groups, "after the rollout")
    _close(A, C)
    # the fused collect
    A, C = _make(label, cfg), _make(label, cfg)
    A.reset()
    obs = _advance([A], acts[:t0])
    C.set_state(*A.get_state())
    torch.manual_seed(5)
    ac = MLPActorCritic(obs_dim=A.obs_dim).cuda()
    ca = collect(A, FusedActorCritic(ac, seed=7), K, obs=obs.clone(), fuse=True)
    cc = collect(C, FusedActorCritic(ac, seed=7), K, obs=obs.clone(), fuse=True)
    assert A.last_collect_fused is True and C.last_collect_fused is True, "the fused collect kernel did not run"
    print(f"{label} ({n} envs): auto-resets inside the fused window: rollout {int(da.sum())}, collect {int(ca.done.sum())}")
    _check_equal(cc, ca)
    _same_state(C, A, groups, "after the fused collect")
    _close(A, C)


@pytest.mark.parametrize("label,size", [("s1-n1d1-gust", "small"), ("s1-n1d1-gust", "large"), ("s2-n1d1", "small")])
def test_import_into_a_running_env(gpu, label, size):
    """load_checkpoint's route: the importing env D has stepped on other actions, so its lanes hold
    the latency ring in its compact form (one stored row and a flag bit that exists in memory only).
    It imports A's state right after A's reset, whose ring rows were drawn one by one, and continues
    as A does: the import writes explicit rows and clears the bit."""
    n = _count(label, size)
    cfg = config(label, n)
    acts = torch.from_numpy(actions(n, 12)).cuda()
    A, D = _make(label, cfg), _make(label, cfg)
    L = A.layout
    A.reset()
    D.reset()
    _advance([D], acts[8:])
    sf, si = A.get_state()
    assert not bool((sf[L.f_abuf:L.f_abuf + 4] == sf[L.f_abuf + 4:L.f_abuf + 8]).all()), "the reset's ring rows are equal"
    D.set_state(sf, si)
    for t in range(8):
        _same_outputs(_step(D, acts[t]), _step(A, acts[t]), f"env-step {t}")
    _same_state(D, A, state_fields(cfg), "after env-step 7")
    _close(A, D)


@pytest.mark.parametrize("label,size", [("s1-n1d1-gust", "small"), ("s1-n1d1-gust", "large"), ("s0-n1d1-agg1", "small"),
                                        ("simple-n1d1", "small"), ("s2-n1d1", "large")])
def test_import_ignores_unused_obs_prev_entries(gpu, label, size):
    """With sensor noise o_{k-1} has 13 entries; the snapshot's entries 13..16 (fields 69..72) mean
    nothing, and the restatement exports them as zero.  A fresh env that imports A's state with those
    entries zeroed continues as A does: the gyro low-pass state comes from its own fields alone."""
    n = _count(label, size)
    cfg = config(label, n)
    assert cfg.observation_noise_on
    T, t0 = horizon(label)
    T = t0 + 6
    acts = torch.from_numpy(actions(n, T)).cuda()
    A, C = _make(label, cfg), _make(label, cfg)
    L = A.layout
    A.reset()
    _advance([A], acts[:t0])
    sf, si = A.get_state()
    assert bool((sf[L.f_lpf:L.f_lpf + 3] != 0).any()), "the low-pass state is still zero"
    sf[L.f_obs_prev + 13:L.f_obs_prev + 17] = 0.0
    C.set_state(sf, si)
    for t in range(t0, T):
        _same_outputs(_step(C, acts[t]), _step(A, acts[t]), f"env-step {t}")
    _same_state(C, A, state_fields(cfg), f"after env-step {T - 1}")
    _close(A, C)
