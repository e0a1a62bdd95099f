"""Data-parallel updates without a GPU: the torch paths of cf2sim.ppo and the running statistics on
two gloo ranks against one process on all rows, and the ABI of the native entry points.

One spawn of two processes runs everything (``ranks``): a synthetic rollout [T = 6, N = 61, D = 34] in
float64, envs split 31 / 30.  Every rank averages with ``all_reduce``, each rank's mean weighted by
its row count, so the ragged split gives the mean over all rows and the results agree with one
process to rounding: 1e-10 relative, in the weights (per tensor, of its largest element) and in every
logged value.  One value mini-batch per pass, so that the ranks' own permutations and the single
process's cover the same rows per step.  The Fisher-vector product takes every row (fvp_stride = 1):
with a stride each rank takes every fourth of its *own* rows, as each process of the reference does,
which is another sample of rows than one process's every fourth.  The parent builds the module and the
rollout once and hands them to the ranks through a file: the synthetic rollout's actions come from an
fp32 forward pass, whose last bits may depend on the process's thread count.
"""
import copy
import dataclasses
import datetime
import os
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_natural_gradient import cast_rollout
from test_ppo_update import CLIP, synthetic_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cf2_ppo_partial_doubles", "cf2_ppo_policy_partial", "cf2_ppo_value_partial", "cf2_ppo_fisher_partial",
         "cf2_ppo_reduce", "cf2_column_moments_partial", "cf2_moments_combine")
T, N, SPLIT, SEED = 6, 61, 31, 3
REL = 1e-10


def rollout64():
    ac, ro = synthetic_rollout(SEED, T=T, N=N)
    g = torch.Generator().manual_seed(77)
    dret = torch.randn(T, N, generator=g) * 2.0 + 5.0
    # logp_old away from the module's own logp: at ratio = 1 LossPi is -mean(A) = 0 up to rounding, and a
    # relative bound on a rounding residue would say nothing
    ro = dataclasses.replace(ro, discounted_ret=dret, logp=ro.logp + 0.1 * torch.randn(T, N, generator=g))
    return ac.double(), cast_rollout(ro, torch.float64)


def shard(ro, rank):
    """The envs [0, 31) or [31, 61) of every [T, N, ...] (and [N, ...]) tensor."""
    from cf2sim.rollout import Rollout
    sl = slice(0, SPLIT) if rank == 0 else slice(SPLIT, N)
    out = {}
    for f in dataclasses.fields(ro):
        if f.name == "storage":
            continue
        t = getattr(ro, f.name)
        out[f.name] = (t[sl] if f.name in ("last_obs", "last_val") else t[:, sl]).contiguous()
    return Rollout(**out)


def make_ppo(ac, group=None):
    from cf2sim.ppo import PPOUpdater
    return PPOUpdater(ac, torch.optim.Adam(ac.pi_net.parameters(), lr=3e-4), torch.optim.Adam(ac.v_net.parameters(), lr=1e-3),
                      CLIP, 1e9, train_pi_iterations=4, train_v_iterations=2, num_mini_batches=1, device=False,
                      generator=torch.Generator().manual_seed(5), group=group)


def make_ng(ac, group=None):
    from cf2sim.ppo import NaturalGradientUpdater
    return NaturalGradientUpdater(ac, 1e-3, 0.01, algorithm="trpo", cg_iters=4, line_search_steps=4, fvp_stride=1,
                                  train_v_iterations=2, num_mini_batches=1, device=False,
                                  generator=torch.Generator().manual_seed(5), group=group)


def run_all(ac0, ro, group, rank=0):
    """The three things under test on one rollout (a shard under a group), each from a copy of the module
    ac0; plain tensors and dicts."""
    from cf2sim.rollout import rank_moments_torch, update_running_statistics
    out = {}
    for name, make in (("ppo", make_ppo), ("ng", make_ng)):
        ac = copy.deepcopy(ac0)
        out[name] = make(ac, group).update(ro)
        out[name + "_weights"] = [p.detach().clone() for p in ac.parameters()]
    ac = copy.deepcopy(ac0).float()
    ro32 = cast_rollout(ro, torch.float32)
    update_running_statistics(ac, ro32, group=group)
    update_running_statistics(ac, ro32, group=group)          # a second batch: the fold into a non-empty state
    out["stats"] = {k: [o.mean.clone(), o.std.clone(), o.count.clone()] for k, o in (("obs", ac.obs_oms), ("ret", ac.ret_oms))}
    if group is not None:
        x = ro32.obs.reshape(-1, ro32.obs.shape[-1]).clone()
        x[:, 3] = 1000.0 + 0.01 * torch.randn(x.shape[0], generator=torch.Generator().manual_seed(10 + rank))
        cnt, mean, m2 = rank_moments_torch(x, group)
        out["moments"] = (cnt, mean, m2)
        out["moments_x"] = x
        empty = x[:0] if rank == 1 else x                      # a rank without rows is skipped
        out["moments_one_empty"] = rank_moments_torch(empty, group)
    return out


def _worker(rank, world, store, out_dir):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    torch.set_num_threads(2)
    ac0, ro = torch.load(os.path.join(out_dir, "data.pt"), weights_only=False)
    out = run_all(ac0, shard(ro, rank), dist.group.WORLD, rank)
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def data():
    return rollout64()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory, data):
    d = tmp_path_factory.mktemp("dp_cpu")
    torch.save(data, d / "data.pt")
    mp.spawn(_worker, args=(2, str(d / "store"), str(d)), nprocs=2, join=True)
    return [torch.load(d / f"rank{r}.pt", weights_only=False) for r in range(2)]


@pytest.fixture(scope="module")
def single(data):
    return run_all(data[0], data[1], None)


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    den = float(b.abs().max())
    return float((a - b).abs().max()) / den if den > 0 else float((a - b).abs().max())


@pytest.mark.parametrize("name", ["ppo", "ng"])
def test_two_ranks_torch_path_agrees_with_one_process(ranks, single, data, name):
    r0, r1 = ranks
    assert r0[name] == r1[name], (r0[name], r1[name])        # the ranks: the same bits
    for a, b in zip(r0[name + "_weights"], r1[name + "_weights"]):
        assert torch.equal(a, b)
    worst = 0.0
    for k, v in single[name].items():
        e = abs(r0[name][k] - v) / abs(v) if v != 0 else abs(r0[name][k])
        worst = max(worst, e)
        assert e <= REL, (name, k, r0[name][k], v)
    before = [p.detach() for p in data[0].parameters()]
    moved = 0
    for a, b, w0 in zip(r0[name + "_weights"], single[name + "_weights"], before):
        worst = max(worst, rel(a, b))
        assert rel(a, b) <= REL
        moved += int(not torch.equal(b, w0))
    print(f"{name}: worst relative difference, two ranks against one process: {worst:.2e}")
    assert moved >= 12                                         # both networks were updated (log_std is not trained)
    if name == "ppo":
        assert single[name]["StopIter"] == 4
    else:
        assert single[name]["AcceptanceStep"] >= 1


def test_two_ranks_running_statistics_are_those_of_the_concatenation(ranks, single, data):
    r0, r1 = ranks
    for k in ("obs", "ret"):
        for a, b, c in zip(r0["stats"][k], r1["stats"][k], single["stats"][k]):
            assert torch.equal(a, b)                           # every rank carries the same statistics
    # one process folding the fp64 two-pass moments of the concatenation into the same starting
    # statistics, twice: the ranks' fp32 buffers may differ from it by the rounding of the combined
    # moments (1e-10) ahead of the one rounding to fp32, i.e. by at most one ulp
    ac, ro = copy.deepcopy(data[0]).float(), data[1]
    for k, oms, x in (("obs", ac.obs_oms, ro.obs.reshape(-1, 34)), ("ret", ac.ret_oms, ro.discounted_ret.reshape(-1, 1))):
        x = x.float().double()
        start = float(oms.count)
        for _ in range(2):
            oms.update_from_moments(T * N, x.mean(0), ((x - x.mean(0)) ** 2).sum(0))
        m0, s0, c0 = r0["stats"][k]
        assert torch.equal(c0, oms.count) and float(c0) == start + 2.0 * T * N
        np.testing.assert_allclose(m0.numpy(), oms.mean.numpy(), rtol=0, atol=2.0 ** -23 * float(oms.mean.abs().max()))
        np.testing.assert_allclose(s0.numpy(), oms.std.numpy(), rtol=2.0 ** -23)
        # and the single process's own torch path (fp32 passes over the rows) to fp32 accuracy
        ms, ss, cs = single["stats"][k]
        assert torch.equal(cs, c0)
        np.testing.assert_allclose(m0.numpy(), ms.numpy(), rtol=0, atol=1e-5 * float(ss.max()))
        np.testing.assert_allclose(s0.numpy(), ss.numpy(), rtol=1e-5)
    # the combined moments against numpy fp64 two-pass over the concatenation (test_epoch_stats.py's bound)
    x = torch.cat([r0["moments_x"], r1["moments_x"]]).double().numpy()
    mean_ref, std_ref = x.mean(0), x.std(0)
    m2_ref = ((x - mean_ref) ** 2).sum(0)
    for r in (r0, r1):
        cnt, mean, m2 = r["moments"]
        assert cnt == T * N and isinstance(cnt, int)
        assert (np.abs(mean.numpy() - mean_ref) <= 1e-10 * np.abs(mean_ref) + 1e-10 * std_ref).all()
        np.testing.assert_allclose(m2.numpy(), m2_ref, rtol=1e-10, atol=0)       # the 1000 +- 0.01 column included
    assert torch.equal(r0["moments"][1], r1["moments"][1]) and torch.equal(r0["moments"][2], r1["moments"][2])
    # a rank without rows: the other rank's moments, bit for bit, on both
    x0 = r0["moments_x"].double()
    for r in (r0, r1):
        cnt, mean, m2 = r["moments_one_empty"]
        assert cnt == T * SPLIT and torch.equal(mean, x0.mean(0)) and torch.equal(m2, ((x0 - x0.mean(0)) ** 2).sum(0))


def test_group_none_is_todays_path():
    """No group: no collective, the updaters' earlier arithmetic (the reducer is inactive)."""
    from cf2sim.dist import RankReducer
    r = RankReducer(None)
    assert (r.world, r.rank, r.active) == (1, 0, False) and RankReducer.of(r) is r
    b = torch.arange(5, dtype=torch.float64)
    g = r.gather(b)
    assert g.shape == (1, 5) and g.data_ptr() == b.data_ptr()
    assert RankReducer(None, force=True).active
    ac, ro = synthetic_rollout(SEED)
    up = make_ppo(ac)
    assert not up.reducer.active and len(up.value_minibatches(7, torch.device("cpu"))) == 1
    forced = make_ppo(copy.deepcopy(ac), RankReducer(None, force=True))
    forced.num_mini_batches = 16
    mbs = forced.value_minibatches(7, torch.device("cpu"))     # across ranks: 16 pieces, some empty
    assert len(mbs) == 16 and sorted(torch.cat(mbs).tolist()) == list(range(7))


def test_abi_declares_and_exports_the_data_parallel_entry_points():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    lib = _native.load()
    txt = open(os.path.join(ROOT, "include", "cf2sim.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(cf2_\w+)\s*\(", txt, flags=re.M))
    for name in NAMES:
        assert name in declared and name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.cf2_abi_version() == 8                       # additive change
    assert lib.cf2_ppo_partial_doubles(35) == 0
    for d in (34, 42):
        assert lib.cf2_ppo_partial_doubles(d) == 8 + d * 64 + 64 + 64 * 64 + 64 + 64 + 1


def test_host_error_paths_need_no_device():
    import ctypes
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    lib = _native.load()
    host = (ctypes.c_double * 64)()                         # never dereferenced: every call returns first
    p = ctypes.addressof(host)
    p += -p % 16
    pol = lambda **kw: lib.cf2_ppo_policy_partial(*[kw.get(k, v) for k, v in (
        ("w", p), ("d", 34), ("obs", p), ("act", p), ("lp", p), ("adv", p), ("n", 8), ("idx", None), ("m", 8), ("mom", None),
        ("cnt", None), ("clip", 0.2), ("mu_old", None), ("mu_out", None), ("logp_out", None), ("with_grad", 1), ("partial", p),
        ("scratch", p), ("ctrl", None), ("stream", None))])
    val = lambda **kw: lib.cf2_ppo_value_partial(*[kw.get(k, v) for k, v in (
        ("w", p), ("d", 34), ("obs", p), ("target", p), ("n", 8), ("idx", None), ("m", 8), ("val_out", None), ("with_grad", 1),
        ("partial", p), ("scratch", p), ("ctrl", None), ("stream", None))])
    fis = lambda **kw: lib.cf2_ppo_fisher_partial(*[kw.get(k, v) for k, v in (
        ("w", p), ("d", 34), ("obs", p), ("n", 8), ("idx", None), ("m", 8), ("vec", p), ("partial", p), ("scratch", p),
        ("ctrl", None), ("stream", None))])
    red = lambda **kw: lib.cf2_ppo_reduce(*[kw.get(k, v) for k, v in (
        ("blocks", p), ("world", 2), ("d", 34), ("value", 0), ("grad", p), ("summary", p), ("ctrl", None), ("stream", None))])
    comb = lambda **kw: lib.cf2_moments_combine(*[kw.get(k, v) for k, v in (
        ("blocks", p), ("world", 2), ("D", 34), ("out", p), ("stream", None))])
    mpart = lambda **kw: lib.cf2_column_moments_partial(*[kw.get(k, v) for k, v in (
        ("x", p), ("rows", 8), ("D", 1), ("block", p), ("scratch", p), ("stream", None))])
    for k in ("w", "obs", "act", "lp", "adv", "partial", "scratch"):
        assert pol(**{k: None}) == -1, k
    for k in ("w", "obs", "target", "partial", "scratch"):
        assert val(**{k: None}) == -1, k
    for k in ("w", "obs", "vec", "partial", "scratch"):
        assert fis(**{k: None}) == -1, k
    assert pol(d=35) == -4 and val(d=35) == -4 and fis(d=35) == -4 and red(d=35) == -4
    assert pol(partial=p + 4) == -1 and val(partial=p + 4) == -1 and fis(partial=p + 4) == -1
    assert pol(act=p + 8) == -1 and pol(obs=p + 4) == -1 and pol(ctrl=p + 2) == -1
    assert pol(mom=p) == -1                                  # moments without the count they were taken over
    assert pol(m=9) == -1 and val(m=9) == -1 and fis(m=9) == -1
    assert pol(m=0, partial=None) == -1                      # m = 0 is legal, but writes the block
    for k in ("blocks", "summary"):
        assert red(**{k: None}) == -1, k
    assert red(world=0) == -1 and red(blocks=p + 4) == -1 and red(summary=p + 4) == -1 and red(grad=p + 2) == -1
    for k in ("blocks", "out"):
        assert comb(**{k: None}) == -1, k
    assert comb(world=0) == -1 and comb(D=0) == -1 and comb(D=65) == -1 and comb(out=p + 4) == -1
    assert mpart(block=None) == -1 and mpart(x=None) == -1 and mpart(D=0) == -1 and mpart(block=p + 4) == -1
    assert lib.cf2_last_hip_error() == 0
