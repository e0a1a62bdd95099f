"""Cost and disturbance level through the fused collect (cf2_collect_step_info,
cf2_collect_rollout_info; collect(..., outcomes=)): the [T, N] cost / level slabs of the one-launch,
one-launch-per-step and two-launch modes are equal bit for bit and equal to step_into's outputs on
the same actions, and every other output of a collect is what it is without ``outcomes``.  N covers
the small kernels (1000: partial 64- and 128-env blocks) and the large one (33 000 > 32 768: the
per-step slab path of cf2_collect_rollout_info, a partial 256-env block).  The reference logs the
level with every episode (episodic_data.csv) and info['cost'] every step (hover_free.py:138-166)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HJ_ENV = "DroneHoverBulletFreeEnvWithRandomHJAdversary-v0"
GUST_ENV = "DroneHoverBulletFreeEnvWithGust-v0"
T = 24
FIELDS = ("obs", "act", "rew", "val", "logp", "done", "trunc", "adv", "ret", "last_obs", "last_val", "trunc_val",
          "discounted_ret")


@functools.lru_cache(maxsize=None)
def _table():
    """One synthetic value table for every level (as tests/test_value_tables.py builds one), on the device."""
    return torch.from_numpy((np.linspace(-1, 1, 15 ** 6, dtype=np.float32) ** 3).reshape(1, -1)).cuda()


def _env(env_id, n):
    from cf2sim.vec_env import BatchedCrazyflieEnv
    e = BatchedCrazyflieEnv(env_id, n, seed=11, want_final_obs=True, max_episode_steps=10)
    if env_id == HJ_ENV:
        e.bind_hj_tables(_table(), [0] * int(e.cfg.num_levels))
    return e


def _policy(obs_dim):
    from cf2sim.rollout import FusedActorCritic, MLPActorCritic
    torch.manual_seed(5)
    ac = MLPActorCritic(obs_dim=obs_dim).cuda()
    with torch.no_grad():
        ac.obs_oms.mean.uniform_(-0.2, 0.2)
        ac.obs_oms.std.uniform_(0.5, 2.0)
        ac.ret_oms.std.fill_(3.0)
    return FusedActorCritic(ac, seed=7, precision="bf16x3")


def _collect(env_id, n, fuse, with_outcomes):
    from cf2sim.rollout import EpisodeStats, LevelOutcomes, collect
    e = _env(env_id, n)
    o = LevelOutcomes.for_env(e) if with_outcomes else None
    st = EpisodeStats(n, e.device) if with_outcomes else None
    r = collect(e, _policy(e.obs_dim), T, fuse=fuse, outcomes=o, stats=st)
    torch.cuda.synchronize()
    assert e.last_collect_fused == fuse, "the collect mode that was asked for did not run"
    state = e.get_state()
    return e, r, o, st, state


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("env_id,n", [(HJ_ENV, 1000), (HJ_ENV, 33000), (GUST_ENV, 1000), (GUST_ENV, 33000)])
def test_collect_info_equals_step_into(gpu, env_id, n):
    from cf2sim.rollout import LevelOutcomes
    runs = {fuse: _collect(env_id, n, fuse, True) for fuse in (True, "steps", False)}
    plain = {fuse: _collect(env_id, n, fuse, False) for fuse in (True, "steps", False)}
    ref = runs[False][1]
    assert ref.cost.shape == ref.level.shape == (T, n) and ref.cost.dtype == ref.level.dtype == torch.float32
    for fuse, (e, r, o, st, state) in runs.items():
        assert _bits(r.cost, ref.cost) and _bits(r.level, ref.level), f"fuse={fuse!r}: cost / level slabs differ"
        # every other output is what collect() gives without outcomes=, bit for bit, and so is the env state
        pe, pr, _, _, pstate = plain[fuse]
        assert pr.cost is None and pr.level is None
        for f in FIELDS:
            a, b = getattr(r, f), getattr(pr, f)
            assert torch.equal(a, b), f"fuse={fuse!r} {f}: max |diff| {(a.float() - b.float()).abs().max().item()}"
        assert torch.equal(state[0], pstate[0]) and torch.equal(state[1], pstate[1])
    # step_into on the same actions, from the same reset: its cost / level outputs are the slabs
    e4 = _env(env_id, n)
    e4.reset()
    obs = torch.empty(n, e4.obs_dim, device=gpu)
    rew, cost, level = (torch.empty(T, n, device=gpu) for _ in range(3))
    done, trunc = (torch.empty(T, n, dtype=torch.uint8, device=gpu) for _ in range(2))
    for t in range(T):
        e4.step_into(ref.act[t].contiguous(), obs, rew[t], done[t], trunc[t], cost[t], level_out=level[t])
    torch.cuda.synchronize()
    assert torch.equal(rew, ref.rew) and torch.equal(done.bool(), ref.done)
    assert _bits(cost, ref.cost) and _bits(level, ref.level)
    # the slabs hold what they should: costs are 0 / 1 flags, levels come from the env's table
    lv = torch.tensor(LevelOutcomes.default_level_values(e4.cfg), dtype=torch.float32, device=gpu)
    assert torch.isin(ref.level, lv).all() and ((ref.cost == 0) | (ref.cost == 1)).all()
    assert ref.done.any() and ref.trunc.any()
    if env_id == HJ_ENV:
        assert ref.level.unique().numel() >= 10, "a Boltzmann-level env draws many levels"
        assert (ref.level[1:] != ref.level[:-1]).any(), "and redraws them at an auto-reset"
        assert (ref.level[1:] != ref.level[:-1])[~ref.done[:-1]].logical_not().all(), "only there"
    else:
        assert lv.numel() == 1 and (ref.level == lv[0]).all()
    # the outcomes of the three modes are one table; it counts the rollout's episodes
    raws = [runs[f][2].raw().cpu() for f in (True, "steps", False)]
    assert torch.equal(raws[0], raws[1]) and torch.equal(raws[0], raws[2])
    s = runs[True][2].summary()
    rows = s["levels"] + [s["other"]]
    assert s["other"]["episodes"] == 0, "every level the env reports is in its table"
    assert sum(e["episodes"] for e in rows) == s["total"]["episodes"] == int(ref.done.sum().item())
    assert all(e["crashes"] + e["timeouts"] == e["episodes"] for e in rows)
    assert s["total"]["timeouts"] == int(ref.trunc.sum().item())
    assert "EpCosts" in s["total"]
    # EpisodeStats got the costs too, and pools the same episodes
    es = runs[True][3].summary()
    assert es["episodes"] == s["total"]["episodes"] and es["EpCosts"]["mean"] == s["total"]["EpCosts"]["mean"]
    assert es["EpRet"]["min"] == s["total"]["EpRet"]["min"] and es["EpLen"]["max"] == s["total"]["EpLen"]["max"]
    for e, *_ in list(runs.values()) + list(plain.values()) + [(e4,)]:
        e.close()


def test_collect_info_reuses_storage_and_continues(gpu):
    """A second collect(out=, obs=) with the same LevelOutcomes re-uses the cost / level slabs and
    carries the running episodes over: the table after both equals one fed by step_into's outputs."""
    from cf2sim.rollout import LevelOutcomes, collect
    n = 1000
    e = _env(HJ_ENV, n)
    p = _policy(e.obs_dim)
    o = LevelOutcomes.for_env(e)
    r1 = collect(e, p, T, outcomes=o)
    c1, l1, rew1, d1, t1 = (x.clone() for x in (r1.cost, r1.level, r1.rew, r1.done, r1.trunc))
    r2 = collect(e, p, T, obs=r1.last_obs, out=r1, outcomes=o)
    assert r2.storage is r1.storage and r2.cost.data_ptr() == r1.cost.data_ptr()
    o2 = LevelOutcomes.for_env(e)
    o2.update(torch.cat([rew1, r2.rew]), torch.cat([d1, r2.done]), torch.cat([t1, r2.trunc]),
              torch.cat([c1, r2.cost]), torch.cat([l1, r2.level]))
    # same episodes, summed in different groupings: both within the summation-order bound of the restatement
    import level_outcomes_reference as R
    cpu = lambda *x: torch.cat(x).cpu().numpy()
    table, abs_sums, *_ = R.level_outcomes(cpu(rew1, r2.rew), cpu(d1, r2.done), o.level_values, cost=cpu(c1, r2.cost),
                                           trunc=cpu(t1, r2.trunc), level=cpu(l1, r2.level))
    R.check_table(o.raw().cpu().numpy(), table, abs_sums)
    R.check_table(o2.raw().cpu().numpy(), table, abs_sums)
    assert table[:, 0].sum() == cpu(d1, r2.done).sum() and table[-1, 0] == 0
    assert torch.equal(o.ep_len, o2.ep_len) and torch.equal(o.ep_ret, o2.ep_ret) and torch.equal(o.ep_cost, o2.ep_cost)
    e.close()


def test_collect_info_entry_points_reject_misaligned(gpu):
    from cf2sim import _native
    n = 1000
    e = _env(GUST_ENV, n)
    p = _policy(e.obs_dim)
    e.reset()
    d = e.obs_dim
    a, a2 = torch.zeros(n, 4, device=gpu), torch.empty(n, 4, device=gpu)
    o, r = torch.empty(n, d, device=gpu), torch.empty(n, device=gpu)
    dn = torch.empty(n, dtype=torch.uint8, device=gpu)
    v, lp = torch.empty(n, device=gpu), torch.empty(n, device=gpu)
    c = torch.full((n + 1,), -3.0, device=gpu)
    for cost, level in ((c.data_ptr() + 2, None), (None, c.data_ptr() + 1)):
        st = e.lib.cf2_collect_step_info(e._ctx, a.data_ptr(), o.data_ptr(), r.data_ptr(), dn.data_ptr(), None, None,
                                         p.w.data_ptr(), d, p.prec, 0, 0, 0, a2.data_ptr(), v.data_ptr(), lp.data_ptr(),
                                         cost, level, e.stream)
        assert st == _native.CF2_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (c == -3.0).all()
    with pytest.raises(ValueError):
        e.collect_step_into(a, o, r, dn, None, None, p, a2, v, lp, cost_out=c)          # [N + 1]
    e.close()
