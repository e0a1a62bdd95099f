"""cf2sim.evaluate.evaluate: exactly ``episodes_per_env`` episodes of every env, however short
(the reference's utils/evaluation.py runs a fixed number of episodes of one env; a batch of
auto-resetting envs needs the quota to do the same)."""
import functools

import numpy as np
import pytest
import torch

import level_outcomes_reference as R

pytestmark = pytest.mark.gpu

ENV = "DroneHoverBulletFreeEnvWithRandomHJAdversary-v0"
N, STEPS, E = 512, 20, 2


@functools.lru_cache(maxsize=None)
def _table():
    return torch.from_numpy((np.linspace(-1, 1, 15 ** 6, dtype=np.float32) ** 3).reshape(1, -1)).cuda()


def _env(env_id=ENV):
    from cf2sim.vec_env import BatchedCrazyflieEnv
    e = BatchedCrazyflieEnv(env_id, N, seed=5, max_episode_steps=STEPS)
    if env_id == ENV:
        e.bind_hj_tables(_table(), [0] * int(e.cfg.num_levels))
    return e


def _module(zero=False):
    from cf2sim.rollout import MLPActorCritic
    torch.manual_seed(2)
    ac = MLPActorCritic(obs_dim=34).cuda()
    if zero:
        with torch.no_grad():
            for p in list(ac.pi_net.parameters()) + list(ac.v_net.parameters()):
                p.zero_()
    return ac


def _rows(out):
    return out["levels"] + [out["other"]]


def test_zero_policy_matches_a_host_side_loop(gpu):
    from cf2sim.evaluate import chunk_bound, evaluate
    from cf2sim.rollout import FusedActorCritic
    e = _env()
    out = evaluate(e, FusedActorCritic(_module(zero=True), seed=1), episodes_per_env=E, chunk=32)
    assert out["total"]["episodes"] == E * N == sum(r["episodes"] for r in _rows(out)) and out["other"]["episodes"] == 0
    assert out["chunks"] <= chunk_bound(E, STEPS, 32) == 2 and out["env_steps"] == 32 * out["chunks"]
    assert all(r["crashes"] + r["timeouts"] == r["episodes"] for r in _rows(out))
    # the same envs stepped with the zero action, scanned on the host with a quota of E per env
    h = _env()
    h.reset()
    T = out["env_steps"]
    act = torch.zeros(N, 4, device=gpu)
    obs = torch.empty(N, h.obs_dim, device=gpu)
    rew, cost, level = (torch.empty(T, N, device=gpu) for _ in range(3))
    done, trunc = (torch.empty(T, N, dtype=torch.uint8, device=gpu) for _ in range(2))
    for t in range(T):
        h.step_into(act, obs, rew[t], done[t], trunc[t], cost[t], level_out=level[t])
    lv = np.array([h.cfg.level_values[k] for k in range(int(h.cfg.num_levels))], dtype=np.float32)
    c = lambda x: x.cpu().numpy()
    table, abs_sums, _, left, eps = R.level_outcomes(c(rew), c(done), lv, cost=c(cost), trunc=c(trunc), level=c(level),
                                                     episodes_left=np.full(N, E, np.int32))
    assert not left.any() and len(eps) == E * N
    assert int(c(done).sum()) > E * N, "without the quota the loop would have counted more episodes of the envs that end early"
    R.check_table(np.array(out["raw"]), table, abs_sums)
    assert [r["episodes"] for r in _rows(out)] == [int(x) for x in table[:, 0]]
    assert sum(1 for r in out["levels"] if r["episodes"]) >= 10, "the episodes spread over the levels"
    # the torch module takes the same actions: the same table, bit for bit
    m = _env()
    out_m = evaluate(m, _module(zero=True), episodes_per_env=E, chunk=32)
    assert out_m["raw"] == out["raw"]
    for x in (e, h, m):
        x.close()


def test_deterministic_twice_and_chunk_bound(gpu):
    from cf2sim.evaluate import chunk_bound, evaluate
    from cf2sim.rollout import FusedActorCritic
    outs = []
    for _ in range(2):
        e = _env()
        outs.append(evaluate(e, FusedActorCritic(_module(), seed=1), episodes_per_env=E, deterministic=True, chunk=8))
        e.close()
    assert outs[0]["raw"] == outs[1]["raw"] and outs[0]["chunks"] == outs[1]["chunks"]
    assert outs[0]["total"]["episodes"] == E * N
    assert outs[0]["chunks"] <= chunk_bound(E, STEPS, 8) == 5
    assert outs[0]["total"]["EpLen"]["max"] <= STEPS


def test_stochastic_and_fixed_level_env(gpu):
    from cf2sim.evaluate import evaluate
    from cf2sim.rollout import FusedActorCritic
    e = _env("DroneHoverBulletFreeEnvWithGust-v0")
    out = evaluate(e, FusedActorCritic(_module(), seed=1), episodes_per_env=3, deterministic=False, chunk=16)
    assert len(out["levels"]) == 1 and out["levels"][0]["level"] == float(np.float32(e.cfg.dstb_level))
    assert out["levels"][0]["episodes"] == out["total"]["episodes"] == 3 * N and out["other"]["episodes"] == 0
    assert out["total"]["crashes"] + out["total"]["timeouts"] == 3 * N
    e.close()


def test_evaluate_needs_a_time_limit(gpu):
    from cf2sim.evaluate import evaluate
    from cf2sim.vec_env import BatchedCrazyflieEnv
    e = BatchedCrazyflieEnv("DroneHoverBulletFreeEnvWithGust-v0", 64, max_episode_steps=0)
    with pytest.raises(ValueError):
        evaluate(e, _module())
    e.close()


def test_cli_writes_json(gpu, tmp_path):
    import json
    from cf2sim.evaluate import main
    torch.save(_module().state_dict(), tmp_path / "w.pt")
    out = tmp_path / "res.json"
    assert main(["--env", "DroneHoverBulletFreeEnvWithGust-v0", "--num-envs", "256", "--weights", str(tmp_path / "w.pt"),
                 "--episodes", "1", "--out", str(out)]) == 0
    res = json.loads(out.read_text())
    assert res["total"]["episodes"] == 256 and res["deterministic"] is True and res["num_envs"] == 256
    assert res["other"]["EpRet"]["mean"] is None, "an empty row's statistics are null in the JSON"
