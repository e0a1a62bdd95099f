"""cf2_level_outcomes (csrc/cf2sim_outcomes.hip) against its NumPy restatement
(tests/level_outcomes_reference.py) on synthetic [T, n] buffers: carries and quota words bit for
bit, counts / crashes / time-outs / min / max exactly, every fp64 sum within the summation-order
bound m * 2^-52 * sum|v|.  The reference is episodic_data.csv's per-level episode log."""
import functools

import numpy as np
import pytest
import torch

import level_outcomes_reference as R

pytestmark = pytest.mark.gpu

NS, TS, LS = (1, 63, 257, 1000), (1, 13, 40), (1, 21, 32)
FOREIGN = (np.float32(7.25), np.float32(-0.0), np.float32(0.05))     # -0.0: the bits differ from 0.0's


def level_table(L):
    if L == 1:
        return np.array([1.5], np.float32)
    if L == 21:
        from cf2sim.config import boltzmann_table
        return boltzmann_table()[0].astype(np.float32)
    return (np.arange(L) * 0.125).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(n, T, L, foreign):
    """Synthetic buffers (read-only): done ~ Bernoulli(0.15), forced at slot 0 and slot T - 1 of some
    envs; trunc a subset of done; levels drawn per slot from the table, ~2 % foreign values when asked."""
    rng = np.random.default_rng(1000 * n + 10 * T + L + (7 if foreign else 0))
    lv = level_table(L)
    rew = (rng.standard_normal((T, n)) * 3.0).astype(np.float32)
    cost = (rng.random((T, n)) < 0.3).astype(np.float32) * rng.integers(1, 4, (T, n)).astype(np.float32)
    done = (rng.random((T, n)) < 0.15).astype(np.uint8)
    done[0, ::3] = 1
    done[T - 1, ::4] = 1
    trunc = (done & (rng.random((T, n)) < 0.4)).astype(np.uint8)
    level = lv[rng.integers(0, L, (T, n))]
    if foreign:
        m = rng.random((T, n)) < 0.02
        m[0, 0] = True                                # slot 0 of env 0 ends an episode: row L is never empty
        level = np.where(m, np.asarray(FOREIGN)[rng.integers(0, len(FOREIGN), (T, n))], level).astype(np.float32)
    for a in (rew, cost, done, trunc, level, lv):
        a.setflags(write=False)
    return rew, cost, done, trunc, level, lv


@functools.lru_cache(maxsize=None)
def reference(n, T, L, foreign):
    rew, cost, done, trunc, level, lv = inputs(n, T, L, foreign)
    return R.level_outcomes(rew, done, lv, cost=cost, trunc=trunc, level=level)


class Run:
    """One set of device carries / table / scratch; call() is one cf2_level_outcomes."""

    def __init__(self, n, L, lv, quota=None):
        from cf2sim import _native
        self.lib, self.native = _native.load(), _native
        self.n, self.L = n, L
        self.lv = torch.from_numpy(np.array(lv)).cuda()
        self.er = torch.zeros(n, device="cuda")
        self.ec = torch.zeros(n, device="cuda")
        self.el = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.left = None if quota is None else torch.full((n,), quota, dtype=torch.int32, device="cuda")
        self.table = torch.full((L + 1, 16), -123.0, dtype=torch.float64, device="cuda")     # overwritten, not read

    def call(self, rew, done, cost=None, trunc=None, level=None, accumulate=0):
        T = rew.shape[0]
        dev = [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in (rew, cost, done, trunc, level)]
        need = self.lib.cf2_level_outcomes_scratch_bytes(T, self.n, self.L)
        assert need > 0
        scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")
        p = self.native.ptr
        st = self.lib.cf2_level_outcomes(T, self.n, p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), p(dev[4]), p(self.lv),
                                         self.L, p(self.er), p(self.ec), p(self.el), p(self.left), p(self.table),
                                         accumulate, p(scratch), torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
        torch.cuda.synchronize()
        return self.table.cpu().numpy()

    def carries(self):
        return self.er.cpu().numpy(), self.ec.cpu().numpy(), self.el.cpu().numpy()


def assert_carries(run, ref_carry):
    for g, r, name in zip(run.carries(), ref_carry, ("ret", "cost", "len")):
        assert g.dtype == r.dtype and np.array_equal(g.view(np.uint32), r.view(np.uint32)), f"carry_{name}"


@pytest.mark.parametrize("foreign", [False, True])
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", NS)
def test_matches_reference(gpu, n, T, L, foreign):
    rew, cost, done, trunc, level, lv = inputs(n, T, L, foreign)
    table, abs_sums, carry, _, eps = reference(n, T, L, foreign)
    # the inputs exercise what they are meant to
    assert eps and (trunc <= done).all() and done[0].any() and done[T - 1].any()
    if T * n >= 63:
        assert trunc.any() and (done & ~trunc).any() and not done.all(), "crashes, time-outs and running steps"
    assert (table[L, 0] > 0) == foreign, "row 'other' is non-empty exactly in the foreign-value cases"
    if (n, T) == (NS[-1], TS[-1]):
        assert (table[:L, 0] >= 2).all(), "every bin holds at least 2 episodes at the largest shape"
        by_env = {}
        for e in eps:
            by_env.setdefault(e[7], set()).add(e[0])
        if L > 1:
            assert any(len(b) >= 2 for b in by_env.values()), "an env ends episodes in different bins within one call"
    run = Run(n, L, lv)
    got = run.call(rew, done, cost, trunc, level)
    R.check_table(got, table, abs_sums)
    assert_carries(run, carry)
    assert table[:, 13].sum() + table[:, 14].sum() == table[:, 0].sum() == len(eps)


@pytest.mark.parametrize("n,T,L", [(1000, 40, 21), (257, 13, 32)])
def test_same_input_same_bits(gpu, n, T, L):
    rew, cost, done, trunc, level, lv = inputs(n, T, L, True)
    runs = [Run(n, L, lv), Run(n, L, lv)]
    tabs = [torch.from_numpy(r.call(rew, done, cost, trunc, level)) for r in runs]
    assert torch.equal(tabs[0].view(torch.int64), tabs[1].view(torch.int64))
    for a, b in zip(runs[0].carries(), runs[1].carries()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n,split", [(1000, 13), (257, 1), (63, 39)])
def test_split_with_accumulate(gpu, n, split):
    T, L = 40, 21
    rew, cost, done, trunc, level, lv = inputs(n, T, L, True)
    table, abs_sums, carry, _, _ = reference(n, T, L, True)
    run = Run(n, L, lv)
    run.call(rew[:split], done[:split], cost[:split], trunc[:split], level[:split], accumulate=0)
    got = run.call(rew[split:], done[split:], cost[split:], trunc[split:], level[split:], accumulate=1)
    assert_carries(run, carry)                       # bit for bit
    R.check_table(got, table, abs_sums)
    # accumulate = 0 overwrites: the second part alone
    part = R.level_outcomes(rew[split:], done[split:], lv, cost=cost[split:], trunc=trunc[split:], level=level[split:],
                            carry=R.level_outcomes(rew[:split], done[:split], lv, cost=cost[:split])[2])
    run2 = Run(n, L, lv)
    run2.call(rew[:split], done[:split], cost[:split], trunc[:split], level[:split], accumulate=1)   # poison rows: count < 0
    got2 = run2.call(rew[split:], done[split:], cost[split:], trunc[split:], level[split:], accumulate=0)
    R.check_table(got2, part[0], part[1])


@pytest.mark.parametrize("quota", [1, 2])
@pytest.mark.parametrize("n,T", [(257, 13), (1000, 13)])
def test_quota_exhausts_inside_a_call(gpu, n, T, quota):
    L = 21
    rew, cost, done, trunc, level, lv = inputs(n, T, L, True)
    ends = done.astype(np.int64).sum(axis=0)
    assert (ends > quota).any() and (ends < quota).any(), "some envs exhaust the quota inside the call, some do not reach it"
    table, abs_sums, carry, left, eps = R.level_outcomes(rew, done, lv, cost=cost, trunc=trunc, level=level,
                                                         episodes_left=np.full(n, quota, np.int32))
    assert len(eps) == np.minimum(ends, quota).sum()
    run = Run(n, L, lv, quota=quota)
    got = run.call(rew, done, cost, trunc, level)
    R.check_table(got, table, abs_sums)
    assert_carries(run, carry)                       # the carries restart at every episode end, recorded or not
    assert np.array_equal(run.left.cpu().numpy(), left)
    # a second call: the exhausted envs record nothing more
    t2, a2, c2, l2, _ = R.level_outcomes(rew, done, lv, cost=cost, trunc=trunc, level=level, carry=carry, episodes_left=left)
    got = run.call(rew, done, cost, trunc, level, accumulate=1)
    R.check_table(got, R.merge_tables(table, t2), abs_sums + a2)
    assert np.array_equal(run.left.cpu().numpy(), l2) and (l2 >= 0).all()
    assert_carries(run, c2)


@pytest.mark.parametrize("drop", ["cost", "trunc", "level", "all"])
def test_null_optionals(gpu, drop):
    n, T, L = 257, 13, 21
    rew, cost, done, trunc, level, lv = inputs(n, T, L, False)
    kw = {"cost": cost, "trunc": trunc, "level": level}
    for k in (("cost", "trunc", "level") if drop == "all" else (drop,)):
        kw[k] = None
    table, abs_sums, carry, _, eps = R.level_outcomes(rew, done, lv, **kw)
    run = Run(n, L, lv)
    got = run.call(rew, done, kw["cost"], kw["trunc"], kw["level"])
    R.check_table(got, table, abs_sums)
    assert_carries(run, carry)
    if kw["trunc"] is None:
        assert got[:, 13].sum() == 0 and got[:, 14].sum() == 0
    if kw["level"] is None:
        assert got[0, 0] == len(eps) and got[1:, 0].sum() == 0
    if kw["cost"] is None:
        assert (got[0, 9:11] == 0).all() and not run.carries()[1].any()


def test_single_level_without_levels(gpu):
    n, T = 1000, 40
    rew, cost, done, trunc, _, lv = inputs(n, T, 1, False)
    table, abs_sums, carry, _, eps = R.level_outcomes(rew, done, lv, cost=cost, trunc=trunc)
    run = Run(n, 1, lv)
    got = run.call(rew, done, cost, trunc, None)
    R.check_table(got, table, abs_sums)
    assert got.shape == (2, 16) and got[0, 0] == len(eps) == done.sum() and got[1, 0] == 0
    assert_carries(run, carry)


def test_errors_write_nothing(gpu):
    from cf2sim import _native
    lib, p = _native.load(), _native.ptr
    n, T, L = 63, 13, 21
    rew, cost, done, trunc, level, lv = inputs(n, T, L, True)
    d = {k: torch.from_numpy(np.array(v)).cuda() for k, v in
         dict(rew=rew, cost=cost, done=done, trunc=trunc, level=level, lv=lv).items()}
    out = dict(er=torch.full((n,), 5.0, device="cuda"), ec=torch.full((n,), 6.0, device="cuda"),
               el=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
               left=torch.full((n,), 9, dtype=torch.int32, device="cuda"),
               table=torch.full((L + 1, 16), -77.0, dtype=torch.float64, device="cuda"),
               scratch=torch.full((lib.cf2_level_outcomes_scratch_bytes(T, n, L) // 8 + 1,), -55.0, dtype=torch.float64,
                                  device="cuda"))
    poison = {k: v.clone() for k, v in out.items()}
    base = dict(T=T, n=n, rew=p(d["rew"]), cost=p(d["cost"]), done=p(d["done"]), trunc=p(d["trunc"]), level=p(d["level"]),
                lv=p(d["lv"]), L=L, er=p(out["er"]), ec=p(out["ec"]), el=p(out["el"]), left=p(out["left"]),
                table=p(out["table"]), acc=0, scratch=p(out["scratch"]))
    order = ("T", "n", "rew", "cost", "done", "trunc", "level", "lv", "L", "er", "ec", "el", "left", "table", "acc", "scratch")

    def call(**edit):
        a = dict(base, **edit)
        st = lib.cf2_level_outcomes(*[a[k] for k in order], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], poison[k]), f"{k} was written by a call that returned {st} for {edit}"
        return st

    for k in ("rew", "done", "lv", "er", "ec", "el", "table", "scratch"):
        assert call(**{k: None}) == _native.CF2_ERR_INVALID_ARG, f"NULL {k}"
    assert call(L=0) == _native.CF2_ERR_INVALID_ARG and call(L=33) == _native.CF2_ERR_INVALID_ARG
    for k in ("rew", "cost", "level", "lv", "er", "ec", "el", "left"):
        assert call(**{k: base[k] + 2}) == _native.CF2_ERR_INVALID_ARG, f"misaligned {k}"
    assert call(table=base["table"] + 4) == _native.CF2_ERR_INVALID_ARG
    assert call(scratch=base["scratch"] + 4) == _native.CF2_ERR_INVALID_ARG
    assert call(T=0) == 0 and call(n=0) == 0, "an empty scan is no error and launches nothing"
    assert lib.cf2_level_outcomes_scratch_bytes(0, n, L) == 0 and lib.cf2_level_outcomes_scratch_bytes(T, n, 33) == 0
    # and the call these were edits of works
    assert lib.cf2_level_outcomes(*[base[k] for k in order], torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert out["table"][:, 0].sum().item() > 0


def test_level_outcomes_class(gpu):
    """cf2sim.rollout.LevelOutcomes over the same buffers: update() in two parts, raw / summary / quota."""
    from cf2sim.rollout import LevelOutcomes
    n, T, L = 257, 40, 21
    rew, cost, done, trunc, level, lv = inputs(n, T, L, True)
    table, abs_sums, carry, _, eps = reference(n, T, L, True)
    o = LevelOutcomes(n, "cuda", lv.astype(np.float64))
    cu = lambda a: torch.from_numpy(np.array(a)).cuda()
    o.update(cu(rew[:7]), cu(done[:7]).bool(), cu(trunc[:7]).bool(), cu(cost[:7]), cu(level[:7]))
    o.update(cu(rew[7:]), cu(done[7:]), cu(trunc[7:]), cu(cost[7:]), cu(level[7:]))
    R.check_table(o.raw().cpu().numpy(), table, abs_sums)
    s = o.summary()
    assert s["total"]["episodes"] == len(eps) and s["other"]["episodes"] == int(table[L, 0]) > 0
    assert [e["episodes"] for e in s["levels"]] == [int(c) for c in table[:L, 0]] and "EpCosts" in s["total"]
    assert o.summary()["total"]["episodes"] == 0, "summary() clears the table"
    assert np.array_equal(o.ep_len.cpu().numpy(), carry[2])
    o.reset()
    o.set_quota(1)
    assert o.remaining() == n
    o.update(cu(rew[0]), cu(done[0]))                 # [N]: one step, no trunc / cost / level
    assert o.remaining() == n - int(done[0].sum())
    s = o.summary()
    assert s["levels"][0]["episodes"] == int(done[0].sum()) and "EpCosts" not in s["total"]
    with pytest.raises(ValueError):
        o.update(cu(rew[:, :5]), cu(done[:, :5]))
