"""Data-parallel updates on the GPU: the rank-partial calls (csrc/cf2sim_ppo.hip), cf2_ppo_reduce and
cf2_moments_combine (csrc/cf2sim_reduce.hip), and the updaters of cf2sim.ppo under a process group.

The kernel tests run in one process with no process group: the shards are row ranges of one buffer,
their partial blocks are stacked in rank order as an all-gather would deliver them.  Shapes: a shard
of 1, 15, 16 or 17 rows sits around one 16-row tile, 47 rows are 3 tiles (less than the PPO_WAVES = 4
of a block), 1000 rows are 16 blocks, 257 rows (the ragged shards of 2049) 5 blocks; a shard of 0 rows
is legal.

Guarantees tested: ranks agree bit for bit (the reduce is a pure function of the gathered blocks, in
rank order); world 1 is the single-rank call bit for bit; another split of the same rows changes
which 16-row tiles share a block's fp32 partial, so its bits differ, and every split meets the
project's rule against fp64 autograd -- per tensor |g - g64|_inf / |g64|_inf <= max(8 x the same
measure of torch's fp32 autograd, 2^-20), summary entries likewise.

Measured on an MI355X over all splits, dense and through a stride-4 index, D = 34 and 42, worst
parameter tensor, kernel / torch-fp32 of that case ("Data-parallel updates"):
policy 3.8e-7 / 5.9e-7, value 8.5e-7 / 1.1e-6, Fisher-vector product 3.0e-7 / 2.7e-7; the worst tensor used
27 % of its bound, the worst summary entry 35 %.  The two-rank steps against fp64, worst policy tensor:
PPO 7.1e-5 (torch fp32: 7.5e-5), TRPO 5.9e-7 (7.3e-7).

The two-rank tests follow tests/test_distributed_gpu.py (mp.spawn, gloo, both ranks on cuda:0) with a
file:// rendezvous under tmp_path and a 60 s group timeout; one spawn per updater.  The parent builds
the module and the rollout once and the ranks load them from a file (the synthetic rollout's actions
come from an fp32 forward pass on the CPU, whose last bits may depend on the thread count).  The data are
chosen so that, in the fp64 reference, every decision is clear of its threshold by a factor of 2 (the
tests assert that): PPO on synthetic_rollout(4): the KL after step 1 is at most target_kl / 2 and after
step 2 at least 2 target_kl (Adam's first two steps are nearly equal, so the KL grows 4.004-fold),
StopIter = 2 of 6; TRPO on synthetic_rollout(3) with target_kl = 3: trial 0 loses 0.095 of the
surrogate (rejected), trial 1 gains 0.138 at KL = 0.43 x 1.5 target_kl (accepted).  The Fisher-vector
product takes every row there (fvp_stride = 1): with a stride every rank takes every fourth of its
own rows, as each process of the reference does, which is another sample than one process's.
"""
import copy
import dataclasses
import datetime
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_natural_gradient import cast_rollout, direction_vec, pi_tensors, same_bits
from test_ppo_update import CLIP, FLOOR, Dev, flat_to_tensors, pool, reference, rel_err, sizes, synthetic_rollout

SPLITS = {"1+16": (1, 16), "15+17": (15, 17), "17+0+1": (17, 0, 1), "1000+1+47": (1000, 1, 47),
          "8x2049": (257, 256, 256, 256, 256, 256, 256, 256)}
assert sum(SPLITS["8x2049"]) == 2049


@pytest.fixture(scope="module")
def lib():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    return _native.load()


def starts(split):
    return [sum(split[:i]) for i in range(len(split))]


def new_block(lib, gpu, d, fill=float("nan"), world=None):
    P = lib.cf2_ppo_partial_doubles(d)
    return torch.full((P,) if world is None else (world, P), fill, dtype=torch.float64, device=gpu)


def shard_partials(lib, gpu, B, kind, split, stride=None, vec=None, with_grad=True, mu_old=True, mom=None, ctrl=None):
    """[world, P]: the partial block of every row range of B's buffers (``stride``: through idx, every
    stride-th row of the shard), in rank order."""
    from cf2sim import ppo
    blocks = new_block(lib, gpu, B.d, world=len(split))
    for r, (s0, cnt) in enumerate(zip(starts(split), split)):
        sl = slice(s0, s0 + cnt)
        idx = None if stride is None else torch.arange(0, cnt, stride, dtype=torch.int32, device=gpu)
        obs = B.obs[sl] if cnt else B.obs[:1]                 # a rank without rows still passes a buffer
        n_kw = {"idx": idx} if idx is not None else ({} if cnt else {"m": 0})
        if kind == "pi":
            take = (lambda t: t[sl]) if cnt else (lambda t: t[:1])
            kw = dict(n_kw)
            if mom is not None:
                kw.update(adv_moments=mom[1:], moments_count=mom[:1])
            ppo.policy_partial_device(B.flat, obs, take(B.act), take(B.logp_old), take(B.adv), CLIP, blocks[r], B.scratch,
                                      with_grad=with_grad, mu_old=take(B.mu_old) if mu_old else None, ctrl=ctrl, **kw)
        elif kind == "v":
            ppo.value_partial_device(B.flat, obs, B.target[sl] if cnt else B.target[:1], blocks[r], B.scratch,
                                     with_grad=with_grad, ctrl=ctrl, **n_kw)
        else:
            ppo.fisher_partial_device(B.flat, obs, vec, blocks[r], B.scratch, ctrl=ctrl, **n_kw)
    return blocks


def split_rows(split, stride):
    return torch.cat([s0 + torch.arange(0, cnt, stride or 1) for s0, cnt in zip(starts(split), split)])


def reference_rows(d, rows, which, dtype, device, adv=None):
    """test_ppo_update.reference on the pool's rows ``rows`` (an index tensor) instead of its first m."""
    from cf2sim.ppo import policy_terms_torch, value_loss_torch
    from test_ppo_update import module_grads
    P = pool(d)
    ac = copy.deepcopy(P["ac"]).to(device=device, dtype=dtype)
    cast = lambda k: P[k][rows].to(device=device, dtype=dtype)
    if which == "pi":
        a = cast("adv") if adv is None else adv.to(device=device, dtype=dtype)
        t = policy_terms_torch(ac, cast("obs"), cast("act"), cast("logp_old"), a, CLIP, mu_old=cast("mu_old"))
        loss = t["rows"].mean()
        loss.backward()
        t = {k: v.detach() for k, v in t.items()}
        summ = [float(len(rows)), float(loss.detach()), float((cast("logp_old") - t["logp"]).mean()),
                float(((t["ratio"] - 1).abs() > CLIP).double().mean()), float(t["kl"].mean()), float(t["ratio"].mean())]
    else:
        loss = value_loss_torch(ac, cast("obs"), cast("target"))
        loss.backward()
        summ = [float(len(rows)), float(loss.detach())]
    return module_grads(ac, which), summ


def assert_rule(label, got, summ, ref64, ref32):
    """The project's rule, per tensor and per summary entry; returns the worst kernel / torch-fp32 pair."""
    (g64, s64), (g32, s32) = ref64, ref32
    ek, e32 = rel_err(got, g64), rel_err(g32, g64)
    print(f"{label}: kernel {max(ek):.3e} torch-fp32 {max(e32):.3e} per tensor {['%.2e' % x for x in ek]} vs "
          f"{['%.2e' % x for x in e32]}")
    for i, (a, b) in enumerate(zip(ek, e32)):
        assert a <= max(8.0 * b, FLOOR), (label, i, a, b)
    ks = summ.tolist()
    assert ks[0] == s64[0] and all(v == 0.0 for v in ks[len(s64):])
    for i in range(1, len(s64)):
        den = abs(s64[i])
        a = abs(ks[i] - s64[i]) / den if den > 0 else abs(ks[i])
        b = abs(s32[i] - s64[i]) / den if den > 0 else abs(s32[i])
        print(f"   summary[{i}] kernel {a:.3e} torch-fp32 {b:.3e}")
        assert a <= max(8.0 * b, FLOOR), (label, "summary", i, ks[i], s64[i], s32[i])
    return max(ek), max(e32)


def fisher_refs(d, rows, dtype, device):
    from cf2sim.ppo import fisher_vec_torch
    P, S = pool(d), sizes(d)
    ac = copy.deepcopy(P["ac"]).to(device=device, dtype=dtype)
    v = direction_vec(d, "random")[:S["pi_end"]].to(device=device, dtype=dtype)
    fv = fisher_vec_torch(ac, P["obs"][rows].to(device=device, dtype=dtype), v)
    return pi_tensors(fv, d), [float(len(rows)), float(torch.dot(v, fv))]


# ---------------------------------------------------------------------------------------------
# 1. world 1 is the existing call, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 17, 1000])
@pytest.mark.parametrize("d", [34, 42])
def test_world_one_is_the_single_rank_call_bit_for_bit(gpu, lib, d, m):
    from cf2sim import ppo
    B = Dev(lib, gpu, d, m)
    S = sizes(d)
    mom = torch.empty(3, dtype=torch.float64, device=gpu)
    cm = torch.empty(lib.cf2_column_moments_scratch_bytes(m, 1) // 8 + 1, dtype=torch.float64, device=gpu)
    adv = (B.adv * 3.0 + 1.5).contiguous()
    ppo.moments_partial_device(adv, mom, cm)
    assert float(mom[0]) == m
    one = lambda: torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
    nan = lambda: torch.full_like(B.flat, float("nan"))
    for with_mu in (False, True):
        for with_mom in (False, True):
            for with_grad in (True, False):
                a = adv if with_mom else B.adv
                mu = B.mu_old if with_mu else None
                g1, s1, g2, s2 = nan(), one(), nan(), one()
                o1 = [torch.full((m, 4), 7.0, device=gpu), torch.full((m,), 7.0, device=gpu)]
                o2 = [t.clone() for t in o1]
                ppo.policy_grad_device(B.flat, B.obs, B.act, B.logp_old, a, CLIP, s1, B.scratch, grad=g1 if with_grad else None,
                                       adv_moments=mom[1:] if with_mom else None, mu_old=mu, mu_out=o1[0], logp_out=o1[1])
                blk = new_block(lib, gpu, d)
                ppo.policy_partial_device(B.flat, B.obs, B.act, B.logp_old, a, CLIP, blk, B.scratch, with_grad=with_grad,
                                          adv_moments=mom[1:] if with_mom else None, moments_count=mom[:1] if with_mom else None,
                                          mu_old=mu, mu_out=o2[0], logp_out=o2[1])
                assert not bool(torch.isnan(blk).any()) and float(blk[0]) == m
                if not with_grad:
                    assert bool((blk[8:] == 0.0).all())          # evaluate only: the head, zeros after it
                ppo.ppo_reduce_device(blk.view(1, -1), d, "pi", s2, grad=g2 if with_grad else None)
                label = (d, m, with_mu, with_mom, with_grad)
                assert same_bits(s1, s2), label
                assert same_bits(g1, g2) and same_bits(o1[0], o2[0]) and same_bits(o1[1], o2[1]), label
                assert bool(torch.isnan(g2[:S["pi_end"]]).any()) != with_grad
    for with_grad in (True, False):
        g1, s1, g2, s2 = nan(), one(), nan(), one()
        v1, v2 = torch.full((m,), 7.0, device=gpu), torch.full((m,), 7.0, device=gpu)
        ppo.value_grad_device(B.flat, B.obs, B.target, s1, B.scratch, grad=g1 if with_grad else None, val_out=v1)
        blk = new_block(lib, gpu, d)
        ppo.value_partial_device(B.flat, B.obs, B.target, blk, B.scratch, with_grad=with_grad, val_out=v2)
        ppo.ppo_reduce_device(blk.view(1, -1), d, "v", s2, grad=g2 if with_grad else None)
        assert same_bits(s1, s2) and same_bits(g1, g2) and same_bits(v1, v2), (d, m, with_grad)
    vec = direction_vec(d, "random").to(gpu)
    g1, s1, g2, s2 = nan(), one(), nan(), one()
    ppo.fisher_vec_device(B.flat, B.obs, vec, g1, s1, B.scratch)
    blk = new_block(lib, gpu, d)
    ppo.fisher_partial_device(B.flat, B.obs, vec, blk, B.scratch)
    ppo.ppo_reduce_device(blk.view(1, -1), d, "pi", s2, grad=g2)
    assert same_bits(s1, s2) and same_bits(g1, g2) and float(s2[1]) > 0


# ---------------------------------------------------------------------------------------------
# 2. splits against fp64
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stride", [None, 4])
@pytest.mark.parametrize("name", list(SPLITS))
@pytest.mark.parametrize("d", [34, 42])
def test_splits_against_fp64(gpu, lib, d, name, stride):
    from cf2sim import ppo
    split = SPLITS[name]
    M = sum(split)
    B = Dev(lib, gpu, d, M)
    rows = split_rows(split, stride)
    vec = direction_vec(d, "random").to(gpu)
    for kind in ("pi", "v", "fisher"):
        blocks = shard_partials(lib, gpu, B, kind, split, stride=stride, vec=vec)
        assert blocks[:, 0].tolist() == [float(len(range(0, c, stride or 1))) for c in split]
        grad = torch.full_like(B.flat, float("nan"))
        summ = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        which = "v" if kind == "v" else "pi"
        ppo.ppo_reduce_device(blocks, d, which, summ, grad=grad)
        if kind == "fisher":
            refs = fisher_refs(d, rows, torch.float64, "cpu"), fisher_refs(d, rows, torch.float32, gpu)
        elif stride is None:
            refs = [reference(d, M, which, dt, dev)[:2] for dt, dev in ((torch.float64, "cpu"), (torch.float32, gpu))]
        else:
            refs = [reference_rows(d, rows, which, dt, dev) for dt, dev in ((torch.float64, "cpu"), (torch.float32, gpu))]
        assert_rule(f"split {name} stride {stride} {kind} d={d}", flat_to_tensors(grad, d, which), summ, *refs)


# ---------------------------------------------------------------------------------------------
# 3. order, determinism, and what a call writes
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", [34, 42])
def test_reduce_is_deterministic_and_any_rank_order_meets_the_rule(gpu, lib, d):
    from cf2sim import ppo
    split = SPLITS["1000+1+47"]
    M = sum(split)
    B = Dev(lib, gpu, d, M)
    S = sizes(d)
    for kind, which in (("pi", "pi"), ("v", "v")):
        blocks = shard_partials(lib, gpu, B, kind, split)
        again = shard_partials(lib, gpu, B, kind, split)
        assert same_bits(blocks, again)                        # the partial: the same input, the same bits
        res = []
        for order in ([0, 1, 2], [0, 1, 2], [2, 1, 0], [1, 2, 0]):
            grad = torch.full_like(B.flat, float("nan"))
            summ = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
            ppo.ppo_reduce_device(blocks[order].contiguous(), d, which, summ, grad=grad)
            res.append((grad, summ))
            refs = [reference(d, M, which, dt, dev)[:2] for dt, dev in ((torch.float64, "cpu"), (torch.float32, gpu))]
            assert_rule(f"order {order} {kind} d={d}", flat_to_tensors(grad, d, which), summ, *refs)
        assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
        print(f"{kind}: a permuted rank order changed bits: {not same_bits(res[0][0], res[2][0])}")
        # the reduce writes exactly its slice and the summary
        lo, hi = (0, S["pi_end"]) if which == "pi" else (S["v_begin"], S["v_end"])
        nan = torch.isnan(res[0][0])
        assert not bool(nan[lo:hi].any()) and bool(nan[:lo].all()) and bool(nan[hi:].all())
        assert not bool(torch.isnan(res[0][1]).any())
        only = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        ppo.ppo_reduce_device(blocks, d, which, only)          # evaluate only: the same summary bits
        assert same_bits(only, res[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("d", [34, 42])
def test_each_partial_call_writes_exactly_its_block(gpu, lib, d):
    from cf2sim import ppo
    B = Dev(lib, gpu, d, 100)
    P = lib.cf2_ppo_partial_doubles(d)
    S = sizes(d)
    npar = {"pi": S["pi_end"], "v": S["v_end"] - S["v_begin"], "fisher": S["pi_end"]}
    vec = direction_vec(d, "random").to(gpu)
    for kind in ("pi", "v", "fisher"):
        pad = torch.full((P + 16,), float("nan"), dtype=torch.float64, device=gpu)
        blk = pad[8:8 + P]
        if kind == "pi":
            ppo.policy_partial_device(B.flat, B.obs, B.act, B.logp_old, B.adv, CLIP, blk, B.scratch)
        elif kind == "v":
            ppo.value_partial_device(B.flat, B.obs, B.target, blk, B.scratch)
        else:
            ppo.fisher_partial_device(B.flat, B.obs, vec, blk, B.scratch)
        assert bool(torch.isnan(pad[:8]).all()) and bool(torch.isnan(pad[8 + P:]).all())
        assert not bool(torch.isnan(blk).any()) and float(blk[0]) == 100.0
        assert bool((blk[8 + npar[kind]:] == 0.0).all()) and bool((blk[8:8 + npar[kind]] != 0.0).any())
        # a rank without rows: a zeroed block from one launch, whatever the other pointers are
        zero = new_block(lib, gpu, d)
        if kind == "pi":
            ppo.policy_partial_device(B.flat, B.obs, B.act, B.logp_old, B.adv, CLIP, zero, B.scratch, m=0)
        elif kind == "v":
            ppo.value_partial_device(B.flat, B.obs, B.target, zero, B.scratch, m=0)
        else:
            ppo.fisher_partial_device(B.flat, B.obs, vec, zero, B.scratch, m=0)
        assert bool((zero == 0.0).all())
    # all ranks without rows: the reduce writes nothing
    grad = torch.full_like(B.flat, float("nan"))
    summ = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
    ppo.ppo_reduce_device(torch.zeros(3, P, dtype=torch.float64, device=gpu), d, "pi", summ, grad=grad)
    assert bool(torch.isnan(grad).all()) and bool((summ == 7.0).all())


# ---------------------------------------------------------------------------------------------
# 4. the gate
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gate_leaves_block_grad_and_summary_untouched(gpu, lib):
    from cf2sim import ppo
    d, m = 34, 100
    B = Dev(lib, gpu, d, m)
    mom = torch.tensor([float(m), 0.1, 90.0], dtype=torch.float64, device=gpu)
    vec = direction_vec(d, "random").to(gpu)
    res = {}
    for flag in (1, 0):
        ctrl = torch.tensor([flag, 0, 0, 0], dtype=torch.int32, device=gpu)
        B.scratch.fill_(-3.0)
        blocks = [shard_partials(lib, gpu, B, "pi", (m,), mom=mom, ctrl=ctrl), shard_partials(lib, gpu, B, "v", (m,), ctrl=ctrl),
                  shard_partials(lib, gpu, B, "fisher", (m,), vec=vec, ctrl=ctrl)]
        if flag:
            assert all(bool(torch.isnan(b).all()) for b in blocks) and bool((B.scratch == -3.0).all())
        good = shard_partials(lib, gpu, B, "pi", (m,), mom=mom)
        grad = torch.full_like(B.flat, float("nan"))
        summ = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        ppo.ppo_reduce_device(good, d, "pi", summ, grad=grad, ctrl=ctrl)
        res[flag] = (grad, summ, blocks[0])
        assert ctrl.tolist() == [flag, 0, 0, 0]                # the launches only read the word
    assert bool(torch.isnan(res[1][0]).all()) and bool((res[1][1] == 7.0).all())
    assert float(res[0][1][0]) == m and not bool(torch.isnan(res[0][0][:sizes(d)["pi_end"]]).any())
    assert same_bits(res[0][2], shard_partials(lib, gpu, B, "pi", (m,), mom=mom))     # an open gate is no gate


# ---------------------------------------------------------------------------------------------
# 5. moments
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SPLITS))
@pytest.mark.parametrize("D", [1, 34])
def test_moments_combine_against_two_pass_fp64(gpu, lib, D, name):
    from cf2sim import ppo
    split = SPLITS[name]
    M = sum(split)
    g = torch.Generator().manual_seed(1000 * D + M)
    x = torch.randn(M, D, generator=g) * 2.0 + 0.5
    x[:, D // 2] = 1000.0 + 0.01 * torch.randn(M, generator=g)
    xd = x.to(gpu)
    scratch = torch.empty(lib.cf2_column_moments_scratch_bytes(M, D) // 8 + 1, dtype=torch.float64, device=gpu)
    blocks = torch.full((len(split), 1 + 2 * D), float("nan"), dtype=torch.float64, device=gpu)
    for r, (s0, cnt) in enumerate(zip(starts(split), split)):
        rows = xd[s0:s0 + cnt]
        ppo.moments_partial_device(rows.reshape(-1) if D == 1 else rows, blocks[r], scratch)
    assert blocks[:, 0].tolist() == [float(c) for c in split] and not bool(torch.isnan(blocks).any())
    out = torch.full((1 + 2 * D,), float("nan"), dtype=torch.float64, device=gpu)
    ppo.moments_combine_device(blocks, out)
    again = torch.full_like(out, float("nan"))
    ppo.moments_combine_device(blocks, again)
    assert same_bits(out, again)
    x64 = x.double().numpy()
    mean_ref, std_ref = x64.mean(0), x64.std(0)
    m2_ref = ((x64 - mean_ref) ** 2).sum(0)
    got = out.cpu().numpy()
    mean, m2 = got[1:1 + D], got[1 + D:]
    assert got[0] == float(M)                                    # count exact
    assert (np.abs(mean - mean_ref) <= 1e-10 * np.abs(mean_ref) + 1e-10 * std_ref).all(), np.abs(mean - mean_ref).max()
    np.testing.assert_allclose(m2, m2_ref, rtol=1e-10, atol=0)   # the 1000 +- 0.01 column included
    # world 1 returns its input bit for bit
    first = next(r for r, c in enumerate(split) if c)
    one = torch.full_like(out, float("nan"))
    ppo.moments_combine_device(blocks[first:first + 1], one)
    assert same_bits(one, blocks[first])
    # blocks of count 0 are ignored, whatever else they hold
    junk = torch.full((1, 1 + 2 * D), float("nan"), dtype=torch.float64, device=gpu)
    junk[0, 0] = 0.0
    with_junk = torch.cat([junk, blocks[:1], junk, blocks[1:], junk]).contiguous()
    other = torch.full_like(out, float("nan"))
    ppo.moments_combine_device(with_junk, other)
    assert same_bits(other, out)
    # against cf2_column_moments on all rows: the same quantity by another grouping
    dense = torch.empty(2 * D, dtype=torch.float64, device=gpu)
    assert lib.cf2_column_moments(xd.data_ptr(), M, D, dense.data_ptr(), scratch.data_ptr(), None) == 0
    np.testing.assert_allclose(got[1 + D:], dense[D:].cpu().numpy(), rtol=2e-10)


# ---------------------------------------------------------------------------------------------
# 6. global advantage standardisation
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_shard_standardises_with_the_moments_of_all_rows(gpu, lib):
    from cf2sim import ppo
    d, split = 34, SPLITS["1000+1+47"]
    M = sum(split)
    B = Dev(lib, gpu, d, M)
    B.adv = (B.adv * 3.0 + 1.5).contiguous()
    mom = torch.empty(3, dtype=torch.float64, device=gpu)      # {count, mean, M2} of all rows
    cm = torch.empty(lib.cf2_column_moments_scratch_bytes(M, 1) // 8 + 1, dtype=torch.float64, device=gpu)
    ppo.moments_partial_device(B.adv, mom, cm)
    a64 = B.adv.double().cpu()
    std = torch.sqrt(((a64 - a64.mean()) ** 2).sum() / M)
    a_std = (a64 - a64.mean()) / (std + 1e-8)
    blocks = shard_partials(lib, gpu, B, "pi", split, mom=mom)
    for r, (s0, cnt) in enumerate(zip(starts(split), split)):
        grad = torch.full_like(B.flat, float("nan"))
        summ = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        ppo.ppo_reduce_device(blocks[r:r + 1], d, "pi", summ, grad=grad)
        rows = torch.arange(s0, s0 + cnt)
        refs = [reference_rows(d, rows, "pi", dt, dev, adv=a_std[rows]) for dt, dev in ((torch.float64, "cpu"), (torch.float32, gpu))]
        assert_rule(f"shard {r} of {split} with the moments of all rows", flat_to_tensors(grad, d, "pi"), summ, *refs)
        # the dense single-rank call on all rows, restricted by idx to the shard's rows: the same tiles of
        # the same rows; the two standardise with sqrt(M2 (n / M) / n) and sqrt(M2 / M), a few fp64 ulp
        # apart, which moves an fp32 advantage by at most one ulp (2^-24 relative) in a few rows
        dense, sd = torch.full_like(B.flat, float("nan")), torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        ppo.policy_grad_device(B.flat, B.obs, B.act, B.logp_old, B.adv, CLIP, sd, B.scratch, grad=dense, adv_moments=mom[1:],
                               mu_old=B.mu_old, idx=rows.to(gpu, dtype=torch.int32))
        e = rel_err(flat_to_tensors(grad, d, "pi"), flat_to_tensors(dense, d, "pi"))
        print(f"   against the dense call through idx: {max(e):.3e}, same bits: {same_bits(grad, dense)}")
        assert max(e) <= FLOOR and float(summ[0]) == float(sd[0]) == cnt


# ---------------------------------------------------------------------------------------------
# 7. error paths launch nothing
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_paths_launch_nothing(gpu, lib):
    d, m = 34, 64
    B = Dev(lib, gpu, d, m)
    P = lib.cf2_ppo_partial_doubles(d)
    blk = torch.full((P + 1,), 7.0, dtype=torch.float64, device=gpu)
    grad = torch.full_like(B.flat, 7.0)
    out = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
    mblk = torch.full((4, 3), 7.0, dtype=torch.float64, device=gpu)
    pad = torch.zeros(64 * 4 + 4, device=gpu)
    act_bad = pad[1:1 + 64 * 4]
    p = lambda t: None if t is None else t.data_ptr()
    odd = lambda t: t.data_ptr() + 4                           # 4 bytes off an 8-byte boundary

    def pol(w=p(B.flat), dim=d, obs=p(B.obs), act=p(B.act), n=m, mm=m, mom=None, cnt=None, partial=p(blk), ctrl=None):
        return lib.cf2_ppo_policy_partial(w, dim, obs, act, p(B.logp_old), p(B.adv), n, None, mm, mom, cnt, CLIP, None, None,
                                          None, 1, partial, p(B.scratch), ctrl, None)

    def val(w=p(B.flat), dim=d, obs=p(B.obs), n=m, partial=p(blk)):
        return lib.cf2_ppo_value_partial(w, dim, obs, p(B.target), n, None, m, None, 1, partial, p(B.scratch), None, None)

    def fis(w=p(B.flat), dim=d, vec=p(B.flat), n=m, partial=p(blk)):
        return lib.cf2_ppo_fisher_partial(w, dim, p(B.obs), n, None, m, vec, partial, p(B.scratch), None, None)

    def red(blocks=p(blk), world=1, dim=d, g=p(grad), summary=p(out)):
        return lib.cf2_ppo_reduce(blocks, world, dim, 0, g, summary, None, None)

    def comb(blocks=p(mblk), world=4, D=1, o=p(out)):
        return lib.cf2_moments_combine(blocks, world, D, o, None)

    assert pol(w=None) == -1 and pol(obs=None) == -1 and pol(partial=None) == -1 and pol(partial=odd(blk)) == -1
    assert pol(act=p(act_bad)) == -1 and pol(n=63) == -1 and pol(dim=35) == -4 and pol(mom=p(out)) == -1
    assert pol(mm=0, partial=None) == -1
    assert val(w=None) == -1 and val(partial=None) == -1 and val(partial=odd(blk)) == -1 and val(n=63) == -1 and val(dim=35) == -4
    assert fis(w=None) == -1 and fis(vec=None) == -1 and fis(partial=odd(blk)) == -1 and fis(n=63) == -1 and fis(dim=35) == -4
    assert red(blocks=None) == -1 and red(summary=None) == -1 and red(world=0) == -1 and red(dim=35) == -4
    assert red(blocks=odd(blk)) == -1 and red(summary=odd(out)) == -1 and red(g=p(grad) + 2) == -1
    assert comb(blocks=None) == -1 and comb(o=None) == -1 and comb(world=0) == -1 and comb(D=0) == -1 and comb(D=65) == -1
    assert comb(blocks=odd(mblk)) == -1 and comb(o=odd(out)) == -1
    assert lib.cf2_column_moments_partial(p(B.adv), m, 1, None, p(B.scratch), None) == -1
    assert lib.cf2_column_moments_partial(None, m, 1, p(mblk), p(B.scratch), None) == -1
    assert lib.cf2_column_moments_partial(p(B.adv), m, 65, p(mblk), p(B.scratch), None) == -1
    torch.cuda.synchronize()
    assert lib.cf2_last_hip_error() == 0
    for t in (blk, grad, out, mblk):
        assert bool((t == 7.0).all())


# ---------------------------------------------------------------------------------------------
# the updaters and the statistics through partial -> gather -> reduce at world 1
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forced_world_one_updaters_are_the_single_rank_updaters_bit_for_bit(gpu, lib):
    from cf2sim.dist import RankReducer
    from cf2sim.ppo import NaturalGradientUpdater, PPOUpdater, ResidentPPOUpdater
    from cf2sim.rollout import pack_policy_weights
    ac0, ro = synthetic_rollout(3, T=6, N=40)
    ro = cast_rollout(ro, device=gpu)
    gen = lambda: torch.Generator(device=gpu).manual_seed(17)
    makers = {
        "resident": lambda ac, g: ResidentPPOUpdater(ac, 3e-4, 1e-3, CLIP, 2e-4, train_pi_iterations=6, train_v_iterations=1,
                                                     generator=gen(), group=g),
        "host loop": lambda ac, g: PPOUpdater(ac, torch.optim.Adam(ac.pi_net.parameters(), lr=3e-4),
                                              torch.optim.Adam(ac.v_net.parameters(), lr=1e-3), CLIP, 2e-4,
                                              train_pi_iterations=6, train_v_iterations=1, generator=gen(), group=g),
        "trpo": lambda ac, g: NaturalGradientUpdater(ac, 1e-3, 3.0, line_search_steps=4, train_v_iterations=1,
                                                     generator=gen(), group=g),
    }
    for name, make in makers.items():
        res = []
        for group in (None, RankReducer(None, force=True)):
            ac = copy.deepcopy(ac0).to(gpu)
            up = make(ac, group)
            assert up.reducer.active == (group is not None)
            res.append((up.update(ro), pack_policy_weights(ac)))
        print(name, res[0][0])
        assert res[0][0] == res[1][0], (name, res[0][0], res[1][0])
        assert same_bits(res[0][1], res[1][1]), name
        assert not same_bits(res[0][1], pack_policy_weights(copy.deepcopy(ac0).to(gpu)))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 34])
def test_update_device_with_a_group_of_one_is_update_device(gpu, lib, d):
    from cf2sim.dist import RankReducer
    from cf2sim.rollout import OnlineMeanStd
    g = torch.Generator().manual_seed(d)
    batches = [(torch.randn(n, d, generator=g) * 3.0 + 7.0).to(gpu) for n in (1000, 17)]
    oms = []
    for group in (None, RankReducer(None, force=True)):
        o = OnlineMeanStd(shape=(d,)).to(gpu)
        for x in batches:
            o.update_device(x.reshape(-1) if d == 1 else x, **({} if group is None else {"group": group}))
        oms.append(o)
    for name in ("mean", "std", "count"):
        assert same_bits(getattr(oms[0], name), getattr(oms[1], name)), name
    assert float(oms[0].count) == 1017.0


# ---------------------------------------------------------------------------------------------
# two ranks on one GPU
# ---------------------------------------------------------------------------------------------
T, N, SPLIT = 6, 61, 31
PPO_SEED, PPO_LR, PPO_TARGET_KL = 4, 3e-4, 4.006e-4
NG_SEED, NG_TARGET_KL = 3, 3.0


def shard(ro, rank):
    from cf2sim.rollout import Rollout
    sl = slice(0, SPLIT) if rank == 0 else slice(SPLIT, N)
    out = {}
    for f in dataclasses.fields(ro):
        if f.name == "storage":
            continue
        t = getattr(ro, f.name)
        out[f.name] = (t[sl] if f.name in ("last_obs", "last_val") else t[:, sl]).contiguous()
    return Rollout(**out)


def make_resident(ac, group=None, gen_seed=17):
    from cf2sim.ppo import ResidentPPOUpdater
    dev = next(ac.parameters()).device
    return ResidentPPOUpdater(ac, PPO_LR, 1e-3, CLIP, PPO_TARGET_KL, train_pi_iterations=6, train_v_iterations=2,
                              num_mini_batches=1, generator=torch.Generator(device=dev).manual_seed(gen_seed), group=group)


def make_torch_ppo(ac, target_kl=PPO_TARGET_KL, iters=6, v_iters=2):
    from cf2sim.ppo import PPOUpdater
    return PPOUpdater(ac, torch.optim.Adam(ac.pi_net.parameters(), lr=PPO_LR), torch.optim.Adam(ac.v_net.parameters(), lr=1e-3),
                      CLIP, target_kl, train_pi_iterations=iters, train_v_iterations=v_iters, num_mini_batches=1, device=False)


def make_ng(ac, device, group=None):
    from cf2sim.ppo import NaturalGradientUpdater
    return NaturalGradientUpdater(ac, 1e-3, NG_TARGET_KL, algorithm="trpo", cg_iters=4, line_search_steps=4, fvp_stride=1,
                                  train_v_iterations=2, num_mini_batches=1, device=device, group=group)


def _worker(rank, world, store, out_dir, which):
    import torch.distributed as dist
    from cf2sim.rollout import pack_policy_weights
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    gpu = torch.device("cuda", 0)
    ac, ro = torch.load(os.path.join(out_dir, "data.pt"), weights_only=False)      # the parent's module and rollout
    ac, ro = ac.to(gpu), cast_rollout(shard(ro, rank), device=gpu)
    if which == "ppo":
        from cf2sim.rollout import update_running_statistics
        twin = copy.deepcopy(ac)
        update_running_statistics(twin, ro, device=True, group=dist.group.WORLD)
        state = {"obs_mean": twin.obs_oms.mean.cpu(), "obs_std": twin.obs_oms.std.cpu(), "obs_count": twin.obs_oms.count.cpu(),
                 "ret_std": twin.ret_oms.std.cpu(), "ret_count": twin.ret_oms.count.cpu()}
        up = make_resident(ac, dist.group.WORLD, gen_seed=17 + rank)       # every rank its own permutations
    else:
        up = make_ng(ac, True, dist.group.WORLD)
    out = up.update(ro)
    if which == "ng":
        state = {"ng_state": up.ng_state.cpu()}
    torch.cuda.synchronize()
    torch.save(dict(state, flat=up.flat.cpu(), module=pack_policy_weights(ac).cpu(), out=out, ctrl=up.ctrl.cpu()),
               os.path.join(out_dir, f"{which}{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def run_two_ranks(tmp_path, which, data):
    torch.save(data, tmp_path / "data.pt")
    mp.spawn(_worker, args=(2, str(tmp_path / "store"), str(tmp_path), which), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"{which}{r}.pt", weights_only=False) for r in range(2))
    for k in r0:                                               # the two ranks: bit for bit
        if isinstance(r0[k], torch.Tensor):
            assert same_bits(r0[k], r1[k]), k
        else:
            assert r0[k] == r1[k], (k, r0[k], r1[k])
    assert same_bits(r0["flat"], r0["module"])
    return r0


def step_rule(label, d, flat_new, flat_old, want, yard):
    """theta_new - theta_old per tensor against fp64, held to 8 x the fp32 torch path's error."""
    got = (flat_new.double() - flat_old.double()).cpu()
    worst = []
    for which in ("pi", "v"):
        g, w, y = (flat_to_tensors(t, d, which) for t in (got, want, yard))
        ek, e32 = rel_err(g, w), rel_err(y, w)
        print(f"{label} {which} step: two ranks {max(ek):.3e} torch-fp32 {max(e32):.3e} per tensor "
              f"{['%.2e' % x for x in ek]} vs {['%.2e' % x for x in e32]}")
        for i, (a, b) in enumerate(zip(ek, e32)):
            assert a <= max(8.0 * b, FLOOR), (label, which, i, a, b)
        worst.append((max(ek), max(e32)))
    return worst


def torch_step(make, data, dtype, dev):
    """(theta_new - theta_old as a flat fp64 block on the CPU, result) of a device=False updater on all rows."""
    ac, ro = copy.deepcopy(data[0]).to(device=dev, dtype=dtype), cast_rollout(data[1], dtype, dev)
    flat64 = lambda: torch.cat([ppo_flat(ac, "pi"), ac.log_std.detach().double().cpu(), ppo_flat(ac, "v"),
                                torch.zeros(2 * 34, dtype=torch.float64)])
    old = flat64()
    out = make(ac).update(ro)
    return flat64() - old, out


def ppo_flat(ac, which):
    from cf2sim.ppo import _linears
    return torch.cat([t.detach().double().cpu().t().reshape(-1) if t.dim() == 2 else t.detach().double().cpu().reshape(-1)
                      for m in _linears(ac, which) for t in (m.weight, m.bias)])


@pytest.mark.gpu
def test_two_ranks_resident_ppo_update(gpu, lib, tmp_path):
    from cf2sim.rollout import pack_policy_weights
    data = synthetic_rollout(PPO_SEED, T=T, N=N)               # built once: the ranks load it from a file
    # the decision in the fp64 reference is clear of its threshold by a factor of 2 on either side
    kl = [torch_step(lambda ac: make_torch_ppo(ac, 1e9, k, 0), data, torch.float64, "cpu")[1]["KL"] for k in (1, 2)]
    print(f"fp64 KL after step 1, 2: {kl[0]:.6e} {kl[1]:.6e}, target_kl {PPO_TARGET_KL:.4e}")
    assert kl[0] <= PPO_TARGET_KL / 2.0 and kl[1] >= 2.0 * PPO_TARGET_KL
    want, ref = torch_step(make_torch_ppo, data, torch.float64, "cpu")
    yard, t32 = torch_step(make_torch_ppo, data, torch.float32, gpu)
    assert ref["StopIter"] == t32["StopIter"] == 2
    r0 = run_two_ranks(tmp_path, "ppo", data)
    ac, ro = copy.deepcopy(data[0]).to(gpu), cast_rollout(data[1], device=gpu)
    old = pack_policy_weights(ac).clone()
    one = make_resident(ac).update(ro)                         # a single process on the concatenated rollout
    print(r0["out"], one, ref)
    assert r0["out"]["StopIter"] == one["StopIter"] == 2 and r0["ctrl"].tolist() == [1, 2, 0, 0]
    for k in ("LossPi", "LossV", "KL"):
        assert abs(r0["out"][k] - ref[k]) <= 1e-4 * max(abs(ref[k]), 1e-3), (k, r0["out"][k], ref[k])
    step_rule("resident ppo", 34, r0["flat"], old.cpu(), want, yard)
    # the running statistics of the two ranks (equal bit for bit, checked above) against one process on all
    # rows: the moments agree to 1e-10 ahead of the one rounding to fp32, so the buffers to one ulp
    from cf2sim.rollout import update_running_statistics
    twin = copy.deepcopy(data[0]).to(gpu)
    update_running_statistics(twin, cast_rollout(data[1], device=gpu), device=True)
    assert torch.equal(r0["obs_count"], twin.obs_oms.count.cpu()) and torch.equal(r0["ret_count"], twin.ret_oms.count.cpu())
    assert float(r0["ret_count"]) == T * N
    mean, std = twin.obs_oms.mean.cpu(), twin.obs_oms.std.cpu()
    assert float((r0["obs_mean"] - mean).abs().max()) <= 2.0 ** -23 * float(mean.abs().max())
    assert float(((r0["obs_std"] - std) / std).abs().max()) <= 2.0 ** -23
    assert not torch.equal(mean, data[0].obs_oms.mean)


@pytest.mark.gpu
def test_two_ranks_natural_gradient_update(gpu, lib, tmp_path):
    import cf2sim.ppo as ppo
    from cf2sim.rollout import pack_policy_weights
    data = synthetic_rollout(NG_SEED, T=T, N=N)
    trials, orig = [], ppo.line_search_torch
    try:
        ppo.line_search_torch = lambda j, total, decay, kl_t, loss, kl, lb: (
            trials.append((j, lb - loss, kl)), orig(j, total, decay, kl_t, loss, kl, lb))[1]
        want, ref = torch_step(lambda ac: make_ng(ac, False), data, torch.float64, "cpu")
    finally:
        ppo.line_search_torch = orig
    print("fp64 trials (trial, improvement, KL):", trials)
    assert ref["AcceptanceStep"] == 2 and len(trials) == 2
    limit = 1.5 * NG_TARGET_KL
    for j, gain, kl in trials:                                 # clear of the accept test by a factor of 2
        if j + 1 == ref["AcceptanceStep"]:
            assert kl <= limit / 2.0 and gain >= 1e-3, (j, gain, kl)
        else:
            assert kl >= 2.0 * limit or gain <= -1e-3, (j, gain, kl)
    yard, t32 = torch_step(lambda ac: make_ng(ac, False), data, torch.float32, gpu)
    r0 = run_two_ranks(tmp_path, "ng", data)
    ac, ro = copy.deepcopy(data[0]).to(gpu), cast_rollout(data[1], device=gpu)
    old = pack_policy_weights(ac).clone()
    one = make_ng(ac, True).update(ro)                         # a single process on the concatenated rollout
    print(r0["out"], one, ref)
    assert r0["out"]["AcceptanceStep"] == one["AcceptanceStep"] == t32["AcceptanceStep"] == 2
    assert r0["ctrl"].tolist() == [1, 2, 0, 0]
    for k in ("LossPi", "KL"):
        assert abs(r0["out"][k] - ref[k]) <= 1e-4 * max(abs(ref[k]), 1e-3), (k, r0["out"][k], ref[k])
    step_rule("trpo", 34, r0["flat"], old.cpu(), want, yard)
