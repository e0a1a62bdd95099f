"""The host side of the per-level outcomes (no GPU): the NumPy restatement of cf2_level_outcomes
against hand-computed cases, LevelOutcomes.merge_raw / table_of, the level CDF against
config.boltzmann_table, evaluate()'s chunk bound and the evaluator's command line."""
import math

import numpy as np
import pytest

import level_outcomes_reference as R


def _f32(*v):
    return np.array(v, dtype=np.float32)


def test_reference_hand_computed():
    # two envs, four steps; env 0: episodes of 2 steps (crash, level 0.5) and 2 steps (time-out, level 1.0);
    # env 1: one episode of 3 steps (crash, a level that is not in the table), then one step still running
    rew = np.array([[1.0, 0.5], [2.0, 0.25], [4.0, 0.125], [8.0, 16.0]], np.float32)
    cost = np.array([[1, 0], [0, 0], [1, 1], [1, 0]], np.float32)
    done = np.array([[0, 0], [1, 0], [0, 1], [1, 0]], np.uint8)
    trunc = np.array([[0, 0], [0, 0], [0, 0], [1, 0]], np.uint8)
    level = np.array([[0.5, 3.0], [0.5, 3.0], [1.0, 3.0], [1.0, 0.5]], np.float32)
    table, abs_sums, (er, ec, el), left, eps = R.level_outcomes(rew, done, _f32(0.5, 1.0), cost=cost, trunc=trunc,
                                                                level=level)
    assert left is None and len(eps) == 3
    assert list(table[0]) == [1, 3.0, 9.0, 3.0, 3.0, 2, 4, 2, 2, 1.0, 1.0, 1.0, 1.0, 1, 0, 0]
    assert list(table[1]) == [1, 12.0, 144.0, 12.0, 12.0, 2, 4, 2, 2, 2.0, 4.0, 2.0, 2.0, 0, 1, 0]
    assert list(table[2]) == [1, 0.875, 0.765625, 0.875, 0.875, 3, 9, 3, 3, 1.0, 1.0, 1.0, 1.0, 1, 0, 0]
    assert list(er) == [0.0, 16.0] and list(ec) == [0.0, 0.0] and list(el) == [0, 1]
    assert list(abs_sums[1]) == [12.0, 144.0, 2.0, 4.0, 2.0, 4.0]


def test_reference_bins_by_bits_and_first_match():
    # -0.0 is not 0.0; a value twice in the table goes to its first entry; level None: row 0
    rew = np.ones((1, 3), np.float32)
    done = np.ones((1, 3), np.uint8)
    level = _f32(-0.0, 0.0, 2.0).reshape(1, 3)
    table, *_ = R.level_outcomes(rew, done, _f32(0.0, 2.0, 2.0), level=level)
    assert list(table[:, 0]) == [1, 1, 0, 1]
    assert list(table[:, 13]) == [0, 0, 0, 0] and list(table[:, 14]) == [0, 0, 0, 0]      # no trunc: no outcome
    assert math.isinf(table[2, 3]) and table[2, 3] > 0 and math.isinf(table[2, 4]) and table[2, 4] < 0
    table, *_ = R.level_outcomes(rew, done, _f32(0.0, 2.0, 2.0))
    assert list(table[:, 0]) == [3, 0, 0, 0]


def test_reference_quota_and_split():
    rng = np.random.default_rng(0)
    rew = rng.standard_normal((12, 5)).astype(np.float32)
    done = (rng.random((12, 5)) < 0.4).astype(np.uint8)
    done[0, 1] = done[11, 2] = 1
    lv = _f32(1.5)
    whole = R.level_outcomes(rew, done, lv, episodes_left=np.full(5, 2, np.int32))
    assert whole[0][0, 0] == sum(min(2, int(done[:, e].sum())) for e in range(5))
    assert list(whole[3]) == [max(0, 2 - int(done[:, e].sum())) for e in range(5)]
    # every recorded episode is one of the env's first two
    for b, ret, ln, cst, crash, tout, t, e in whole[4]:
        assert int(done[:t, e].sum()) < 2
    # a split scan changes no carry and no episode
    a = R.level_outcomes(rew[:5], done[:5], lv)
    b = R.level_outcomes(rew[5:], done[5:], lv, carry=a[2])
    c = R.level_outcomes(rew, done, lv)
    for x, y in zip(b[2], c[2]):
        assert np.array_equal(x, y)
    assert [e[1:4] for e in a[4] + b[4]] == [e[1:4] for e in c[4]]
    R.check_table(R.merge_tables(a[0], b[0]), c[0], c[1])


def test_check_table_is_tight():
    rew = np.array([[1.0, 3.0, 5.0]], np.float32)
    done = np.ones((1, 3), np.uint8)
    table, abs_sums, *_ = R.level_outcomes(rew, done, _f32(1.5))
    R.check_table(table, table, abs_sums)
    # sum 9 (ulp 8 * 2^-52): bound 3 * 9 * 2^-52 = 3.375 ulp; sum of squares 35 (ulp 32 * 2^-52): 3 * 35 * 2^-52 = 3.28 ulp
    for word, delta in ((0, 1.0), (3, 1e-9), (13, 1.0), (1, 4 * 8 * 2.0 ** -52), (2, 4 * 32 * 2.0 ** -52)):
        bad = table.copy()
        bad[0, word] += delta
        assert bad[0, word] != table[0, word]
        with pytest.raises(AssertionError):
            R.check_table(bad, table, abs_sums)
    ok = table.copy()
    ok[0, 1] += 3 * 8 * 2.0 ** -52
    ok[0, 2] -= 3 * 32 * 2.0 ** -52
    assert ok[0, 1] != table[0, 1] and ok[0, 2] != table[0, 2]
    R.check_table(ok, table, abs_sums)


def test_merge_raw_and_table_of():
    from cf2sim.rollout import LevelOutcomes
    rng = np.random.default_rng(1)
    lv = _f32(0.0, 0.5, 1.0)
    parts, eps_all = [], []
    for r in range(3):                    # three "ranks"
        rew = rng.standard_normal((9, 4)).astype(np.float32)
        done = (rng.random((9, 4)) < 0.35).astype(np.uint8)
        trunc = done & (rng.random((9, 4)) < 0.5)
        level = rng.choice(np.append(lv, np.float32(9.0)), size=(9, 4)).astype(np.float32)
        if r == 2:
            level[:] = 0.5                # a rank with empty rows
        cost = (rng.random((9, 4)) < 0.3).astype(np.float32)
        t, _, _, _, eps = R.level_outcomes(rew, done, lv, cost=cost, trunc=trunc, level=level)
        parts.append(t)
        eps_all += eps
    merged = LevelOutcomes.merge_raw(parts).numpy()
    ref, abs_sums = R.table_of(eps_all, 3)
    R.check_table(merged, ref, abs_sums)
    assert merged.shape == (4, 16)
    with pytest.raises(ValueError):
        LevelOutcomes.merge_raw([parts[0], parts[1][:3]])
    with pytest.raises(ValueError):
        LevelOutcomes.merge_raw([])
    out = LevelOutcomes.table_of(merged, lv)
    assert [e["level"] for e in out["levels"]] == [0.0, 0.5, 1.0]
    rows = out["levels"] + [out["other"]]
    for k, e in enumerate(rows):
        mine = [x for x in eps_all if x[0] == k]
        assert e["episodes"] == len(mine) and e["crashes"] + e["timeouts"] == e["episodes"]
        assert e["crashes"] == sum(1 for x in mine if x[4])
        if mine:
            rets = np.array([float(x[1]) for x in mine])
            assert e["crash_rate"] == e["crashes"] / len(mine)
            assert e["EpRet"]["mean"] == pytest.approx(rets.mean(), rel=1e-12, abs=1e-12)
            assert e["EpRet"]["std"] == pytest.approx(rets.std(), rel=1e-9, abs=1e-9)
            assert e["EpRet"]["min"] == rets.min() and e["EpRet"]["max"] == rets.max()
            assert e["EpLen"]["max"] == max(x[2] for x in mine)
            assert e["EpCosts"]["mean"] == pytest.approx(np.mean([float(x[3]) for x in mine]), rel=1e-12)
    tot = out["total"]
    assert tot["episodes"] == len(eps_all) == sum(e["episodes"] for e in rows)
    assert tot["crashes"] == sum(e["crashes"] for e in rows) and tot["timeouts"] == sum(e["timeouts"] for e in rows)
    assert tot["EpRet"]["min"] == min(float(x[1]) for x in eps_all)
    # an empty table: NaN means and rate, no exception; EpCosts only when asked for
    empty = LevelOutcomes.table_of(R.empty_table(3), lv, with_costs=False)
    assert empty["total"]["episodes"] == 0 and math.isnan(empty["total"]["crash_rate"])
    assert math.isnan(empty["levels"][0]["EpRet"]["mean"]) and "EpCosts" not in empty["levels"][0]
    with pytest.raises(ValueError):
        LevelOutcomes.table_of(merged, lv[:2])


def test_default_level_values():
    from cf2sim.config import build_config
    from cf2sim.rollout import LevelOutcomes
    c = build_config("DroneHoverBulletFreeEnvWithRandomHJAdversary-v0", 4)
    lv = LevelOutcomes.default_level_values(c)
    assert len(lv) == int(c.num_levels) == 21 and lv[0] == 0.0 and lv[20] == 2.0
    g = build_config("DroneHoverBulletFreeEnvWithGust-v0", 4)
    assert LevelOutcomes.default_level_values(g) == [float(g.dstb_level)]


def test_level_cdf_matches_boltzmann_table():
    from cf2sim.config import boltzmann_table, build_config, level_cdf_from
    values, cdf = boltzmann_table()
    w = np.exp(-1.0 * np.arange(0.0, 2.1, 0.1))
    p = w / np.sum(w)
    assert level_cdf_from(p) == list(cdf)                       # the same bits as numpy's cumsum and division
    c = build_config("DroneHoverBulletFreeEnvWithRandomHJAdversary-v0", 4)
    assert level_cdf_from(p) == [float(c.level_cdf[k]) for k in range(int(c.num_levels))]
    # unnormalised weights: the division normalises; a weight of 0 repeats the entry before it, and
    # trailing zeros give exactly 1.0, so searchsorted(u, 'right') never lands on such a level for u < 1
    cdf = level_cdf_from([0, 0, 3, 0, 1, 0, 0])
    assert cdf == [0.0, 0.0, 0.75, 0.75, 1.0, 1.0, 1.0]
    us = np.append(np.arange(0, 1 << 24, 4099) * 2.0 ** -24, [0.0, 0.75 - 2.0 ** -24, 0.75, 1 - 2.0 ** -24])   # u01's range
    idx = np.minimum(np.searchsorted(np.array(cdf[:-1]), us, side="right"), 6)     # boltzmann_index: entries k < L - 1
    assert set(idx.tolist()) == {2, 4}
    one_hot = level_cdf_from([0.0] * 20 + [5.0])
    assert one_hot == [0.0] * 20 + [1.0]
    for bad in ([], [0.0, 0.0], [1.0, -0.5], [1.0, math.nan], [1.0, math.inf]):
        with pytest.raises(ValueError):
            level_cdf_from(bad)


def test_chunk_bound():
    from cf2sim.evaluate import chunk_bound
    assert chunk_bound(1, 500, 32) == 16 and chunk_bound(2, 20, 32) == 2 and chunk_bound(2, 20, 8) == 5
    assert chunk_bound(1, 32, 32) == 1 and chunk_bound(1, 33, 32) == 2 and chunk_bound(3, 1, 64) == 1
    for e, m, c in ((2, 20, 32), (5, 500, 7), (1, 1, 1)):
        assert (chunk_bound(e, m, c) - 1) * c < e * m <= chunk_bound(e, m, c) * c
    for bad in ((0, 20, 32), (1, 0, 32), (1, 20, 0)):
        with pytest.raises(ValueError):
            chunk_bound(*bad)


def test_cli_arguments():
    from cf2sim.evaluate import _jsonable, build_parser
    p = build_parser()
    a = p.parse_args(["--env", "DroneHoverBulletFreeEnvWithGust-v0", "--num-envs", "64", "--weights", "w.pt"])
    assert (a.env, a.num_envs, a.weights) == ("DroneHoverBulletFreeEnvWithGust-v0", 64, "w.pt")
    assert a.tables is None and a.episodes == 1 and not a.stochastic and not a.uniform_levels and a.out is None
    a = p.parse_args(["--env", "X", "--num-envs", "8", "--weights", "w.pt", "--tables", "dir", "--episodes", "3",
                      "--stochastic", "--uniform-levels", "--out", "r.json"])
    assert (a.tables, a.episodes, a.stochastic, a.uniform_levels, a.out) == ("dir", 3, True, True, "r.json")
    for missing in (["--num-envs", "8", "--weights", "w.pt"], ["--env", "X", "--weights", "w.pt"],
                    ["--env", "X", "--num-envs", "8"], ["--env", "X", "--num-envs", "many", "--weights", "w.pt"]):
        with pytest.raises(SystemExit):
            p.parse_args(missing)
    assert _jsonable({"a": [math.nan, 1.5, -math.inf], "b": {"c": 2}}) == {"a": [None, 1.5, None], "b": {"c": 2}}


def test_load_policy_reads_both_state_dict_layouts(tmp_path):
    import torch
    from cf2sim.evaluate import load_policy
    from cf2sim.rollout import MLPActorCritic
    torch.manual_seed(0)
    ac = MLPActorCritic(obs_dim=34)
    torch.save(ac.state_dict(), tmp_path / "own.pt")
    ref = {}
    for mine, name in ((ac.pi_net, "pi.net"), (ac.v_net, "v.net")):
        for i in (0, 2, 4):
            ref[f"{name}.{i}.weight"], ref[f"{name}.{i}.bias"] = mine[i].weight.detach(), mine[i].bias.detach()
    ref["pi.log_std"] = ac.log_std.detach()
    torch.save(ref, tmp_path / "ref.pt")
    for f in ("own.pt", "ref.pt"):
        got = load_policy(str(tmp_path / f), 34, "cpu")
        for a, b in zip(got.parameters(), ac.parameters()):
            assert torch.equal(a, b)
