"""Per-epoch training statistics: cf2_episode_stats / cf2_column_moments (csrc/cf2sim_stats.hip),
EpisodeStats, OnlineMeanStd.update_from_moments / update_device and their wiring into collect()
and update_running_statistics().  References are numpy on the host."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cf2_episode_stats_scratch_bytes", "cf2_episode_stats", "cf2_column_moments_scratch_bytes",
         "cf2_column_moments")
ENV_ID = "DroneHoverBulletFreeEnvWithoutAdversary-v0"


@pytest.fixture(scope="module")
def lib():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    return _native.load()


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_statistics_entry_points(lib):
    from cf2sim._native import EXPORTED_SYMBOLS
    txt = open(os.path.join(ROOT, "include", "cf2sim.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(cf2_\w+)\s*\(", txt, flags=re.M))
    for name in NAMES:
        assert name in declared and name in EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.cf2_abi_version() == 8                       # additive change


def test_abi_error_paths_launch_nothing(lib):
    host = (ctypes.c_double * 64)()                         # never dereferenced: every call returns first
    p = ctypes.addressof(host)
    assert lib.cf2_episode_stats(4, 8, *([None] * 10), 1, None, None) == -1
    for missing in (2, 4, 5, 6, 7, 11, 13):                 # rew, done, the carries, summary, scratch
        args = [4, 8, p, None, p, p, p, p, None, None, None, p, 1, p, None]
        args[missing] = None
        assert lib.cf2_episode_stats(*args) == -1, missing
    assert lib.cf2_column_moments(None, 5, 34, None, None, None) == -1
    assert lib.cf2_column_moments(None, 5, 34, p, p, None) == -1
    assert lib.cf2_column_moments(p, 5, 34, None, p, None) == -1
    assert lib.cf2_column_moments(p, 5, 34, p, None, None) == -1
    for d in (0, 65):
        assert lib.cf2_column_moments(p, 5, d, p, p, None) == -1
        assert lib.cf2_column_moments_scratch_bytes(5, d) == 0
    # empty sizes: CF2_OK, and no scratch
    assert lib.cf2_episode_stats(0, 8, *([None] * 10), 1, None, None) == 0
    assert lib.cf2_episode_stats(4, 0, *([None] * 10), 1, None, None) == 0
    assert lib.cf2_column_moments(None, 0, 34, None, None, None) == 0
    assert lib.cf2_episode_stats_scratch_bytes(0) == 0
    assert lib.cf2_column_moments_scratch_bytes(0, 34) == 0
    assert lib.cf2_episode_stats_scratch_bytes(257) > 0 and lib.cf2_episode_stats_scratch_bytes(257) % 8 == 0
    assert lib.cf2_column_moments_scratch_bytes(2 ** 33, 34) > 0


def test_merge_raw_against_a_hand_computed_merge():
    from cf2sim.rollout import EpisodeStats
    inf = math.inf
    #     count  ret: sum sumsq min max   len: sum sumsq min max   cost: sum sumsq min max
    a = [3.0, 6.0, 14.0, 1.0, 3.0, 30.0, 350.0, 5.0, 15.0, 0.5, 0.25, 0.0, 0.5, 0, 0, 0]
    b = [2.0, -4.0, 10.0, -3.0, -1.0, 9.0, 41.0, 4.0, 5.0, 4.0, 8.0, 2.0, 2.0, 0, 0, 0]
    empty = [0.0, 99.0, 99.0, -99.0, 99.0, 9.0, 9.0, 9.0, 9.0, 1.0, 1.0, 1.0, 1.0, 0, 0, 0]   # count 0: ignored
    want = [5.0, 2.0, 24.0, -3.0, 3.0, 39.0, 391.0, 4.0, 15.0, 4.5, 8.25, 0.0, 2.0, 0, 0, 0]
    got = EpisodeStats.merge_raw([torch.tensor(a, dtype=torch.float64), np.array(empty), np.array(b)])
    assert got.dtype == torch.float64 and got.tolist() == want
    none = EpisodeStats.merge_raw([np.array(empty), np.zeros(16)])
    assert none.tolist() == [0.0, 0, 0, inf, -inf, 0, 0, inf, -inf, 0, 0, inf, -inf, 0, 0, 0]
    s = EpisodeStats.summary_of(got)
    assert s["episodes"] == 5
    assert s["EpRet"] == {"mean": 0.4, "std": math.sqrt(24.0 / 5 - 0.4 * 0.4), "min": -3.0, "max": 3.0}
    assert s["EpLen"]["mean"] == 7.8 and s["EpLen"]["min"] == 4.0 and s["EpLen"]["max"] == 15.0
    assert "EpCosts" not in EpisodeStats.summary_of(got, with_costs=False)
    assert EpisodeStats.summary_of(none)["episodes"] == 0


def oms_reference(state, x):
    """OnlineMeanStd.update restated in fp64 numpy (batch variance about the new mean)."""
    mean, std, count = state
    x = np.asarray(x, dtype=np.float64)
    n_b, n_a = x.shape[0], count
    n_ab = n_a + n_b
    delta = x.mean(0) - mean
    mean_new = mean + delta * n_b / n_ab
    batch_var = ((x - mean_new) ** 2).mean(0)
    m2 = n_a * std ** 2 + n_b * batch_var + delta ** 2 * (n_a * n_b / n_ab)
    return mean_new, np.sqrt(m2 / n_ab), n_ab


def oms_batches(d, seed):
    """Two batches with different means and spreads, so the new-mean variance term matters."""
    rng = np.random.default_rng(seed)
    b1 = (rng.normal(size=(700, d)) * rng.uniform(0.5, 2.0, d) + rng.uniform(-3.0, 3.0, d)).astype(np.float32)
    b2 = (rng.normal(size=(1300, d)) * rng.uniform(0.5, 2.0, d) + rng.uniform(2.0, 6.0, d)).astype(np.float32)
    return b1, b2


def oms_check(oms, state, batches, rtol):
    xmax = max(float(np.abs(b).max()) for b in batches)
    np.testing.assert_allclose(oms.mean.double().cpu().numpy().reshape(-1), state[0], rtol=rtol, atol=rtol * xmax)
    np.testing.assert_allclose(oms.std.double().cpu().numpy().reshape(-1), state[1], rtol=rtol, atol=rtol * xmax)
    assert float(oms.count.item()) == state[2]


@pytest.mark.parametrize("d", [5, 1])
def test_update_from_moments_matches_update(d):
    from cf2sim.rollout import OnlineMeanStd
    a, b = OnlineMeanStd(shape=(d,)), OnlineMeanStd(shape=(d,))
    keys = list(a.state_dict().keys())
    state = (np.zeros(d), np.ones(d), 0.0)
    batches = oms_batches(d, seed=d)
    for i, x in enumerate(batches):
        x64 = x.astype(np.float64)
        mean_b = x64.mean(0)
        m2_b = ((x64 - mean_b) ** 2).sum(0)
        a.update_from_moments(x.shape[0], torch.from_numpy(mean_b), torch.from_numpy(m2_b))
        b.update(torch.from_numpy(x.reshape(-1) if d == 1 else x))
        state = oms_reference(state, x)
        oms_check(a, state, batches[:i + 1], 1e-6)          # fp64 rounded once into the fp32 buffers
        oms_check(b, state, batches[:i + 1], 1e-4)          # the fp32 update: guards the formula only
    assert list(a.state_dict().keys()) == keys and a.mean.dtype == a.std.dtype == a.count.dtype == torch.float32
    assert a.mean.shape == (d,) and a.std.shape == (d,) and a.count.shape == (1,)
    with pytest.raises(ValueError):
        a.update_from_moments(0, torch.zeros(d), torch.zeros(d))


# ---------------------------------------------------------------------------------------------
# on the GPU: episode kernel
# ---------------------------------------------------------------------------------------------
def episode_reference(rew, cost, done, carry=None):
    """Per-env loop with np.float32 adds.  Returns the carries, the per-slot outputs (prefilled with
    -7) and the finished episodes' (return, length, cost) in scan order."""
    T, n = rew.shape
    cr, cc, cl = carry if carry is not None else (np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32))
    cr, cc, cl = cr.copy(), cc.copy(), cl.copy()
    o_ret, o_len, o_cost = np.full((T, n), -7, np.float32), np.full((T, n), -7, np.int32), np.full((T, n), -7, np.float32)
    eps = []
    for e in range(n):
        r, c, l = cr[e], cc[e], cl[e]
        for t in range(T):
            r = np.float32(r + rew[t, e])
            c = np.float32(c + cost[t, e])
            l = l + 1
            if done[t, e]:
                o_ret[t, e], o_len[t, e], o_cost[t, e] = r, l, c
                eps.append((r, l, c))
                r, c, l = np.float32(0), np.float32(0), 0
        cr[e], cc[e], cl[e] = r, c, l
    return (cr, cc, cl), (o_ret, o_len, o_cost), eps


class EpisodeRun:
    """Device state of a sequence of cf2_episode_stats calls."""

    def __init__(self, lib, n, dev):
        self.lib, self.n, self.dev = lib, n, dev
        self.cr = torch.zeros(n, device=dev)
        self.cc = torch.zeros(n, device=dev)
        self.cl = torch.zeros(n, dtype=torch.int32, device=dev)
        self.summary = torch.zeros(16, dtype=torch.float64, device=dev)
        self.scratch = torch.empty(lib.cf2_episode_stats_scratch_bytes(n) // 8, dtype=torch.float64, device=dev)

    def call(self, rew, cost, done, outs, accumulate):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        r, c, d = t(rew), (t(cost) if cost is not None else None), t(done.astype(np.uint8))
        st = self.lib.cf2_episode_stats(rew.shape[0], self.n, r.data_ptr(), c.data_ptr() if c is not None else None,
                                        d.data_ptr(), self.cr.data_ptr(), self.cc.data_ptr(), self.cl.data_ptr(),
                                        *[o.data_ptr() if o is not None else None for o in outs],
                                        self.summary.data_ptr(), accumulate, self.scratch.data_ptr(),
                                        torch.cuda.current_stream(self.dev).cuda_stream)
        assert st == 0
        torch.cuda.synchronize(self.dev)

    def carries(self):
        return self.cr.cpu().numpy(), self.cc.cpu().numpy(), self.cl.cpu().numpy()


def new_outs(T, n, dev):
    return (torch.full((T, n), -7.0, device=dev), torch.full((T, n), -7, dtype=torch.int32, device=dev),
            torch.full((T, n), -7.0, device=dev))


def check_summary(s, eps):
    """s: 16 doubles from the device; eps: the reference's finished episodes."""
    assert s[0] == len(eps) and (s[13:] == 0).all()
    for k, col in ((1, 0), (5, 1), (9, 2)):
        if not eps:
            assert s[k] == 0 and s[k + 1] == 0 and s[k + 2] == math.inf and s[k + 3] == -math.inf
            continue
        v = np.array([e[col] for e in eps]).astype(np.float64)      # the same f32 / int values
        assert s[k + 2] == v.min() and s[k + 3] == v.max()
        if col == 1:
            assert s[k] == v.sum() and s[k + 1] == (v * v).sum()     # integers: exact
        else:
            # reordered fp64 sums of <= 3e3 terms: n 2^-53 ~ 3e-13
            np.testing.assert_allclose(s[k], v.sum(), rtol=1e-12)
            np.testing.assert_allclose(s[k + 1], (v * v).sum(), rtol=1e-12)


def episode_inputs(T, n, kind, seed):
    rng = np.random.default_rng(seed)
    rew = rng.normal(size=(T, n)).astype(np.float32)
    cost = rng.normal(size=(T, n)).astype(np.float32)
    done = {"random": rng.random((T, n)) < 0.1, "ones": np.ones((T, n), bool), "zeros": np.zeros((T, n), bool)}[kind]
    return rew, cost, done


@pytest.mark.gpu
@pytest.mark.parametrize("T,n,kind", [(29, 1000, "random"), (1, 257, "random"), (8, 1, "random"), (17, 64, "ones"),
                                      (29, 300, "zeros")])
def test_episode_kernel_matches_the_per_env_loop(gpu, lib, T, n, kind):
    rew, cost, done = episode_inputs(T, n, kind, seed=T * 1000 + n)
    if (T, n) == (8, 1):
        done[5, 0] = True                                            # at least one episode in the tiny case
    carry, outs_ref, eps = episode_reference(rew, cost, done)
    run = EpisodeRun(lib, n, gpu)
    outs = new_outs(T, n, gpu)
    run.call(rew, cost, done, outs, accumulate=0)
    for got, want in zip(run.carries(), carry):
        assert np.array_equal(got, want)
    for got, want in zip(outs, outs_ref):                            # set slots and the untouched -7 slots
        assert np.array_equal(got.cpu().numpy(), want)
    check_summary(run.summary.cpu().numpy(), eps)
    if kind == "ones":
        assert run.summary[0].item() == T * n and run.summary[7].item() == 1 and run.summary[8].item() == 1
    if kind == "zeros":
        assert np.array_equal(run.carries()[2], np.full(n, T, np.int32))
    # cost_dev == NULL is cost 0 everywhere; no per-slot outputs wanted
    run2 = EpisodeRun(lib, n, gpu)
    run2.call(rew, None, done, (None, None, None), accumulate=0)
    s2 = run2.summary.cpu().numpy()
    assert np.array_equal(run2.carries()[0], carry[0]) and not run2.carries()[1].any()
    assert np.array_equal(s2[:9], run.summary.cpu().numpy()[:9])
    assert list(s2[9:13]) == ([0, 0, 0, 0] if eps else [0, 0, math.inf, -math.inf])


@pytest.mark.gpu
def test_episode_kernel_is_split_invariant_and_deterministic(gpu, lib):
    T, n = 29, 1000
    rew, cost, done = episode_inputs(T, n, "random", seed=77)
    _, _, eps = episode_reference(rew, cost, done)
    one = EpisodeRun(lib, n, gpu)
    outs1 = new_outs(T, n, gpu)
    one.call(rew, cost, done, outs1, accumulate=0)
    two = EpisodeRun(lib, n, gpu)
    outs2 = new_outs(T, n, gpu)
    two.summary.fill_(123.0)
    two.summary[0] = 0.0                                             # count 0: empty whatever else it holds
    two.call(rew[:11], cost[:11], done[:11], [o[:11] for o in outs2], accumulate=1)
    two.call(rew[11:], cost[11:], done[11:], [o[11:] for o in outs2], accumulate=1)
    for a, b in zip(one.carries(), two.carries()):
        assert np.array_equal(a, b)
    for a, b in zip(outs1, outs2):
        assert torch.equal(a, b)
    s1, s2 = one.summary.cpu().numpy(), two.summary.cpu().numpy()
    exact = [0, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15]                # count, min, max, lengths
    assert np.array_equal(s1[exact], s2[exact])
    np.testing.assert_allclose(s2[[1, 2, 9, 10]], s1[[1, 2, 9, 10]], rtol=1e-12)
    check_summary(s2, eps)
    # accumulate = 0 overwrites whatever the summary held
    two.cr.zero_(), two.cc.zero_(), two.cl.zero_()
    two.call(rew[:11], cost[:11], done[:11], (None, None, None), accumulate=0)
    first = EpisodeRun(lib, n, gpu)
    first.call(rew[:11], cost[:11], done[:11], (None, None, None), accumulate=0)
    assert two.summary[0].item() == done[:11].sum()
    assert np.array_equal(two.summary.cpu().numpy()[exact], first.summary.cpu().numpy()[exact])
    # two identical calls on fresh state: identical bits
    again = EpisodeRun(lib, n, gpu)
    again.call(rew, cost, done, (None, None, None), accumulate=0)
    assert np.array_equal(again.summary.cpu().numpy().view(np.uint64), s1.view(np.uint64))


# ---------------------------------------------------------------------------------------------
# on the GPU: column moments
# ---------------------------------------------------------------------------------------------
def moments_matrix(rows, d, seed, kind=None):
    """N(0, 1) columns, one column at 1000 + 0.01 N(0, 1) and one constant column (a single column:
    the one `kind` names)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(rows, d)).astype(np.float32)
    offset = (1000.0 + 0.01 * rng.normal(size=rows)).astype(np.float32)
    if d == 1:
        if kind == "offset":
            x[:, 0] = offset
        elif kind == "const":
            x[:, 0] = np.float32(-2.75)
        return x, ([0] if kind == "offset" else []), ([0] if kind == "const" else [])
    x[:, d // 3] = offset
    x[:, d - 2] = np.float32(3.14159)
    return x, [d // 3], [d - 2]


def device_moments(lib, x_dev, rows, d):
    out = torch.full((2 * d,), -1.0, dtype=torch.float64, device=x_dev.device)
    scratch = torch.empty(lib.cf2_column_moments_scratch_bytes(rows, d) // 8, dtype=torch.float64, device=x_dev.device)
    st = lib.cf2_column_moments(x_dev.data_ptr(), rows, d, out.data_ptr(), scratch.data_ptr(),
                                torch.cuda.current_stream(x_dev.device).cuda_stream)
    assert st == 0
    o = out.cpu().numpy()
    return o[:d], o[d:]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,d,kind", [(1, 34, None), (29000, 34, None), (4097, 42, None), (100003, 1, "normal"),
                                         (100003, 1, "offset"), (100003, 1, "const"), (5001, 13, "view"),
                                         (4097, 34, "view8")])
def test_column_moments_match_two_pass_fp64(gpu, lib, rows, d, kind):
    x, offset_cols, const_cols = moments_matrix(rows, d, seed=rows + d, kind=kind)
    if kind in ("view", "view8"):                                    # base 4-byte / 8-byte aligned only
        off = 1 if kind == "view" else 2
        flat = torch.zeros(off + rows * d, device=gpu)
        flat[off:] = torch.from_numpy(x.reshape(-1)).to(gpu)
        xd = flat[off:].view(rows, d)
        assert xd.data_ptr() % 16 == 4 * off
    else:
        xd = torch.from_numpy(x).to(gpu)
        assert xd.data_ptr() % 16 == 0
    mean, m2 = device_moments(lib, xd, rows, d)
    x64 = x.astype(np.float64)
    mean_ref = x64.mean(0)
    m2_ref = ((x64 - mean_ref) ** 2).sum(0)
    std_ref = np.sqrt(m2_ref / rows)
    # fp64 accumulation: n 2^-53 <= 1.2e-11 at n <= 1.1e5, about x8 margin
    assert (np.abs(mean - mean_ref) <= 1e-10 * np.abs(mean_ref) + 1e-10 * std_ref).all(), np.abs(mean - mean_ref).max()
    np.testing.assert_allclose(m2, m2_ref, rtol=1e-10, atol=0)       # the 1000 +- 0.01 column included
    assert (m2 >= 0).all()
    for c in const_cols:
        assert m2[c] == 0.0 and mean[c] == x64[0, c]
    for c in offset_cols:
        assert rows == 1 or abs(m2[c] / rows - 1e-4) < 2e-5          # the column is what it should be
    mean_b, m2_b = device_moments(lib, xd, rows, d)
    assert np.array_equal(mean.view(np.uint64), mean_b.view(np.uint64))
    assert np.array_equal(m2.view(np.uint64), m2_b.view(np.uint64))


@pytest.mark.gpu
def test_column_moments_index_past_2_to_32_elements(gpu, lib):
    """rows is 64-bit: a constant [2^31 + 3, 2] matrix (2^32 + 6 elements, 17 GB) whose last row
    differs.  The moments are known in closed form, and they come out only if the last elements are
    reached: mean = 1.5 + delta / rows, M2 = delta^2 (rows - 1) / rows."""
    rows, d = 2 ** 31 + 3, 2
    x = torch.full((rows, d), 1.5, device=gpu)
    x[-1, 0], x[-1, 1] = 2.5, -0.5
    mean, m2 = device_moments(lib, x, rows, d)
    del x
    torch.cuda.empty_cache()
    for c, delta in ((0, 1.0), (1, -2.0)):
        np.testing.assert_allclose(mean[c], 1.5 + delta / rows, rtol=1e-15)
        np.testing.assert_allclose(m2[c], delta * delta * (rows - 1) / rows, rtol=1e-10)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [34, 1])
def test_update_device_matches_the_fp64_restatement(gpu, d):
    from cf2sim.rollout import OnlineMeanStd
    oms = OnlineMeanStd(shape=(d,)).to(gpu)
    state = (np.zeros(d), np.ones(d), 0.0)
    batches = oms_batches(d, seed=40 + d)
    for i, x in enumerate(batches):
        oms.update_device(torch.from_numpy(x.reshape(-1) if d == 1 else x).to(gpu))
        state = oms_reference(state, x)
        oms_check(oms, state, batches[:i + 1], 1e-6)
    assert sorted(oms.state_dict().keys()) == ["count", "mean", "std"]
    with pytest.raises(ValueError):
        oms.update_device(torch.zeros(4, d + 1, device=gpu))
    with pytest.raises(ValueError):
        oms.update_device(torch.zeros(4, 2 * d, device=gpu)[:, ::2] if d > 1 else torch.zeros(8, device=gpu)[::2])


# ---------------------------------------------------------------------------------------------
# on the GPU: end to end
# ---------------------------------------------------------------------------------------------
def running_returns(rew, done, cost=None):
    """np.float32 running sums along every env of [T, N] buffers: the finished episodes' returns (and
    costs, lengths) with their slots."""
    z = np.zeros_like(rew) if cost is None else cost
    _, (o_ret, o_len, o_cost), eps = episode_reference(rew, z, done)
    return o_ret, o_len, o_cost, eps


@pytest.mark.gpu
def test_collect_follows_episodes_across_two_fused_collects(gpu):
    from cf2sim.rollout import EpisodeStats, FusedActorCritic, MLPActorCritic, collect, update_running_statistics
    from cf2sim.vec_env import BatchedCrazyflieEnv
    torch.manual_seed(0)
    n, T = 512, 48
    envs = BatchedCrazyflieEnv(ENV_ID, n, seed=5, want_final_obs=True, max_episode_steps=20)
    ac = MLPActorCritic().to(gpu)
    fused = FusedActorCritic(ac, seed=1)
    st = EpisodeStats(n, gpu)
    ro1 = collect(envs, fused, T, stats=st)
    ro2 = collect(envs, fused, T, obs=ro1.last_obs, stats=st)
    raw = st.raw().cpu().numpy()
    # the same buffers through a second EpisodeStats, with the per-slot outputs
    st2 = EpisodeStats(n, gpu)
    outs = new_outs(2 * T, n, gpu)
    st2.update(ro1.rew, ro1.done, ep_ret_out=outs[0][:T], ep_len_out=outs[1][:T], ep_cost_out=outs[2][:T])
    st2.update(ro2.rew, ro2.done, ep_ret_out=outs[0][T:], ep_len_out=outs[1][T:], ep_cost_out=outs[2][T:])
    assert np.array_equal(st2.raw().cpu().numpy().view(np.uint64), raw.view(np.uint64))
    rew = torch.cat([ro1.rew, ro2.rew]).cpu().numpy()
    done = torch.cat([ro1.done, ro2.done]).cpu().numpy()
    o_ret, o_len, _, eps = running_returns(rew, done)
    assert np.array_equal(outs[0].cpu().numpy(), o_ret)              # every finished episode's return, exactly
    assert np.array_equal(outs[1].cpu().numpy(), o_len)
    assert done[T - 1].sum() < n and (o_len[T:][done[T:]] > np.nonzero(done[T:])[0] + 1).any()   # some span the cut
    s = st.summary()
    assert s["episodes"] == int(done.sum()) == len(eps) and s["episodes"] > n
    assert s["EpLen"]["max"] <= 20 and s["EpLen"]["min"] >= 1
    assert "EpCosts" not in s                                        # the fused path has no cost output
    rets = np.array([e[0] for e in eps], np.float64)
    assert s["EpRet"]["min"] == rets.min() and s["EpRet"]["max"] == rets.max()
    np.testing.assert_allclose(s["EpRet"]["mean"], rets.mean(), rtol=1e-9)
    np.testing.assert_allclose(s["EpRet"]["std"], rets.std(), rtol=1e-6)
    np.testing.assert_allclose(s["EpLen"]["mean"], np.mean([e[1] for e in eps]), rtol=1e-12)
    assert st.summary()["episodes"] == 0                             # cleared; the carries stay
    assert np.array_equal(st.ep_len.cpu().numpy(), st2.ep_len.cpu().numpy()) and st.ep_len.any()
    # update_running_statistics(device=True) against the torch update on a copy
    ac_t = MLPActorCritic().to(gpu)
    ac_t.load_state_dict(ac.state_dict())
    update_running_statistics(ac, ro2, fused, device=True)
    update_running_statistics(ac_t, ro2)
    for a, b in ((ac.obs_oms, ac_t.obs_oms), (ac.ret_oms, ac_t.ret_oms)):
        torch.testing.assert_close(a.mean, b.mean, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(a.std, b.std, rtol=1e-4, atol=1e-5)
        assert torch.equal(a.count, b.count)
    st.reset(torch.arange(n, device=gpu) % 2 == 0)
    assert not st.ep_len[::2].any() and torch.equal(st.ep_len[1::2], st2.ep_len[1::2])
    with pytest.raises(ValueError):
        st.update(ro1.rew[:, :5], ro1.done[:, :5])
    with pytest.raises(ValueError):
        st.update(ro1.rew.double(), ro1.done)
    envs.close()


@pytest.mark.gpu
def test_collect_torch_path_reports_episode_costs(gpu):
    from cf2sim.rollout import EpisodeStats, MLPActorCritic, collect
    from cf2sim.vec_env import BatchedCrazyflieEnv
    torch.manual_seed(0)
    n, T = 64, 24
    make = lambda: BatchedCrazyflieEnv(ENV_ID, n, seed=9, want_final_obs=True, max_episode_steps=10)
    envs, ac = make(), MLPActorCritic().to(gpu)
    st = EpisodeStats(n, gpu)
    ro = collect(envs, ac, T, generator=torch.Generator(device=gpu).manual_seed(3), stats=st)
    s = st.summary()
    # the same actions through a second env of the same seed: its info["cost"], summed the same way
    twin = make()
    twin.reset()
    cost = np.zeros((T, n), np.float32)
    for t in range(T):
        _, r, _, info = twin.step(ro.act[t].contiguous())
        assert torch.equal(r, ro.rew[t])
        cost[t] = info["cost"].cpu().numpy()
    _, _, _, eps = running_returns(ro.rew.cpu().numpy(), ro.done.cpu().numpy(), cost)
    assert s["episodes"] == len(eps) == int(ro.done.sum().item()) and s["episodes"] >= 2 * n
    costs = np.array([e[2] for e in eps], np.float64)
    assert s["EpCosts"]["min"] == costs.min() and s["EpCosts"]["max"] == costs.max()
    np.testing.assert_allclose(s["EpCosts"]["mean"], costs.mean(), rtol=1e-12, atol=1e-300)
    rets = np.array([e[0] for e in eps], np.float64)
    assert s["EpRet"]["min"] == rets.min() and s["EpRet"]["max"] == rets.max()
    # one update without costs since the clear: no EpCosts
    st.update(ro.rew, ro.done, ro.rew)
    st.update(ro.rew, ro.done)
    assert "EpCosts" not in st.summary() and "EpCosts" in st.summary()
    envs.close()
    twin.close()


@pytest.mark.gpu
def test_collect_with_stats_changes_no_rollout_tensor(gpu):
    from cf2sim.rollout import EpisodeStats, FusedActorCritic, MLPActorCritic, collect
    from cf2sim.vec_env import BatchedCrazyflieEnv
    torch.manual_seed(0)
    n, T = 256, 24
    ac = MLPActorCritic().to(gpu)
    fields = ("obs", "act", "rew", "val", "logp", "done", "trunc", "adv", "ret", "last_obs", "last_val", "trunc_val",
              "discounted_ret")
    for use_fused in (True, False):
        ros = []
        for stats in (None, EpisodeStats(n, gpu)):
            envs = BatchedCrazyflieEnv(ENV_ID, n, seed=11, want_final_obs=True, max_episode_steps=10)
            pol = FusedActorCritic(ac, seed=4) if use_fused else ac
            g = None if use_fused else torch.Generator(device=gpu).manual_seed(8)
            ros.append(collect(envs, pol, T, generator=g, stats=stats))
            torch.cuda.synchronize()
            envs.close()
        for f in fields:
            assert torch.equal(getattr(ros[0], f), getattr(ros[1], f)), (use_fused, f)
