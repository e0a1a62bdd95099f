"""The PPO update: cf2_ppo_policy_grad / cf2_ppo_value_grad (csrc/cf2sim_ppo.hip) and cf2sim.ppo
(torch restatements of the two losses, scatter_flat_grad, the device wrappers, PPOUpdater).

The reference of every GPU test is torch autograd in fp64 on the same inputs.  Tolerance rule of the
gradient tests: per parameter tensor the error is |g - g64|_inf / |g64|_inf; the kernel may be at most
8 x the same measure of torch's fp32 autograd (its summation order differs: tiles, blocks, fp64
merge), with a floor of 2^-20.  Summary entries are held to the same rule relative to their fp64
values.  Measured on an MI355X, worst parameter tensor, kernel / torch-fp32 (the full table is in
DESIGN.md section 8, "The PPO update on the device"):

    m        policy D=34          policy D=42          value D=34           value D=42
    1        2.8e-7 / 5.2e-7      3.0e-7 / 1.8e-7      2.3e-7 / 2.4e-7      1.8e-7 / 1.8e-7
    15       2.3e-7 / 3.4e-7      2.3e-7 / 2.7e-7      1.0e-6 / 7.7e-7      2.3e-7 / 2.5e-7
    17       2.3e-7 / 3.3e-7      2.6e-7 / 2.1e-7      9.5e-7 / 1.1e-6      2.3e-7 / 3.0e-7
    1000     1.9e-7 / 4.8e-7      1.7e-7 / 5.9e-7      2.6e-7 / 9.7e-7      2.1e-7 / 1.2e-6
    70001    7.3e-8 / 2.1e-6      7.1e-8 / 1.7e-6      5.3e-8 / 2.6e-6      6.0e-8 / 3.5e-6

Inputs (``pool``): torch-initialised weights, observation statistics away from (0, 1), logp_old from
a perturbed copy of the policy so that rows fall on both sides of the clip range with both advantage
signs.  Rows within 1e-4 of the clip kinks (ratio = 1 +- c) or with a hidden ReLU pre-activation
|z| < 1e-5 are dropped before any call (fp32 and fp64 may legitimately take different branches
there); ``test_pool_covers_the_cases`` checks without a GPU that at most 1 % are dropped and that
each of the four (clipped or not) x (A > 0 or A < 0) cases holds >= 5 % of the rows, of the pool and
of its first 1000 rows (the m >= 1000 cases; a prefix of 1, 15 or 17 rows cannot hold four 5 % shares).

The kernel's grid is at most 512 blocks of 4 waves, 16 rows per wave and pass, so m = 70 001 > 32 768
makes waves run more than one tile, as the issue's 512 x 8-wave grid does at that m.
"""
import copy
import ctypes
import functools
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cf2_ppo_scratch_bytes", "cf2_ppo_policy_grad", "cf2_ppo_value_grad")
ENV_ID = "DroneHoverBulletFreeEnvWithoutAdversary-v0"
CLIP = 0.2
FLOOR = 2.0 ** -20
POOL = 70001
MS = (1, 15, 17, 1000, 70001)


@pytest.fixture(scope="module")
def lib():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    return _native.load()


def sizes(d):
    """(begin, in, out) of W and begin of b per layer in the flat block, pi then v."""
    out, off = {}, 0
    for which, h, no in (("pi", 50, 4), ("v", 64, 1)):
        layers = []
        for i, o in ((d, h), (h, h), (h, no)):
            layers.append((off, i, o, off + i * o))
            off += i * o + o
        out[which] = layers
        if which == "pi":
            out["pi_end"] = off
            off += 4
    out["v_begin"], out["v_end"] = out["v"][0][0], off
    return out


def flat_to_tensors(flat, d, which):
    """The slice's tensors in torch's shapes: [W1, b1, W2, b2, W3, b3]."""
    res = []
    for w_off, i, o, b_off in sizes(d)[which]:
        res += [flat[w_off:w_off + i * o].view(i, o).t(), flat[b_off:b_off + o]]
    return res


def module_grads(ac, which):
    net = ac.pi_net if which == "pi" else ac.v_net
    return [p.grad for m in net if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]


def make_ac(d, seed):
    from cf2sim.rollout import MLPActorCritic
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    ac = MLPActorCritic(obs_dim=d)
    with torch.no_grad():
        ac.obs_oms.mean.copy_(torch.randn(d, generator=g) * 0.5)
        ac.obs_oms.std.copy_(torch.rand(d, generator=g) * 1.5 + 0.5)
        ac.obs_oms.count.fill_(1000.0)
    return ac


def pi_preacts(ac64, obs64):
    from cf2sim.ppo import _standardized
    z1 = ac64.pi_net[0](_standardized(ac64, obs64))
    z2 = ac64.pi_net[2](torch.relu(z1))
    return torch.cat([z1, z2], dim=1)


@functools.lru_cache(maxsize=None)
def pool(d):
    """Inputs of the gradient tests, built once per obs_dim on the CPU (fp64 where it decides a case)."""
    from cf2sim.ppo import policy_terms_torch
    g = torch.Generator().manual_seed(100 + d)
    ac = make_ac(d, seed=d)
    n0 = POOL + POOL // 50
    obs = (ac.obs_oms.mean + ac.obs_oms.std * torch.randn(n0, d, generator=g)).float()
    old = copy.deepcopy(ac)
    with torch.no_grad():
        for p in old.pi_net.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.03)
        ac64, old64 = copy.deepcopy(ac).double(), copy.deepcopy(old).double()
        o64 = obs.double()
        z = torch.zeros(n0, dtype=torch.float64)
        mu_old = policy_terms_torch(old64, o64, torch.zeros(n0, 4, dtype=torch.float64), z, z, CLIP)["mu"]
        act = (mu_old + 0.5 * torch.randn(n0, 4, generator=g).double()).float()
        logp_old = policy_terms_torch(old64, o64, act.double(), z, z, CLIP)["logp"].float()
        adv = torch.randn(n0, generator=g)
        target = torch.randn(n0, generator=g)
        t = policy_terms_torch(ac64, o64, act.double(), logp_old.double(), adv.double(), CLIP)
        near_clip = ((t["ratio"] - (1 - CLIP)).abs() < 1e-4) | ((t["ratio"] - (1 + CLIP)).abs() < 1e-4)
        near_relu = (pi_preacts(ac64, o64).abs() < 1e-5).any(dim=1)
        keep = ~(near_clip | near_relu)
        dropped = float((~keep[:POOL]).double().mean())
        sel = keep.nonzero().squeeze(1)[:POOL]
        assert sel.numel() == POOL
        ratio, a = t["ratio"][sel], adv[sel].double()
        clipped = ((a > 0) & (ratio > 1 + CLIP)) | ((a < 0) & (ratio < 1 - CLIP))
    return {"ac": ac, "obs": obs[sel].contiguous(), "act": act[sel].contiguous(), "logp_old": logp_old[sel].contiguous(),
            "adv": adv[sel].contiguous(), "target": target[sel].contiguous(), "mu_old": mu_old[sel].float().contiguous(),
            "dropped": dropped, "clipped": clipped, "pos": a > 0}


def rel_err(got, want):
    """per tensor |got - want|_inf / |want|_inf (inf where want is 0 and got is not)."""
    out = []
    for x, w in zip(got, want):
        x, w = x.detach().double().cpu(), w.detach().double().cpu()
        den, num = float(w.abs().max()), float((x - w).abs().max())
        out.append(num / den if den > 0 else (0.0 if num == 0 else math.inf))
    return out


def reference(d, m, which, dtype, device, adv=None):
    """(gradient tensors, summary values) of torch autograd in `dtype` on the pool's first m rows."""
    from cf2sim.ppo import policy_terms_torch, value_loss_torch
    P = pool(d)
    ac = copy.deepcopy(P["ac"]).to(device=device, dtype=dtype)
    cast = lambda k: P[k][:m].to(device=device, dtype=dtype)
    for p in ac.parameters():
        p.grad = None
    if which == "pi":
        a = cast("adv") if adv is None else adv.to(device=device, dtype=dtype)
        t = policy_terms_torch(ac, cast("obs"), cast("act"), cast("logp_old"), a, CLIP, mu_old=cast("mu_old"))
        loss = t["rows"].mean()
        loss.backward()
        t = {k: v.detach() for k, v in t.items()}
        summ = [float(m), float(loss.detach()), float((cast("logp_old") - t["logp"]).mean()),
                float(((t["ratio"] - 1).abs() > CLIP).double().mean()), float(t["kl"].mean()), float(t["ratio"].mean())]
        extra = {"mu": t["mu"], "logp": t["logp"]}
    else:
        loss = value_loss_torch(ac, cast("obs"), cast("target"))
        loss.backward()
        summ = [float(m), float(loss.detach())]
        extra = {}
    return module_grads(ac, which), summ, extra


class Dev:
    """Device buffers of one (obs_dim, m) case."""

    def __init__(self, lib, gpu, d, m, n=None):
        from cf2sim.rollout import pack_policy_weights
        P = pool(d)
        n = m if n is None else n
        self.d, self.m, self.n = d, m, n
        self.flat = pack_policy_weights(P["ac"]).to(gpu)
        for k in ("obs", "act", "logp_old", "adv", "target", "mu_old"):
            setattr(self, k, P[k][:n].to(gpu).contiguous())
        self.summary = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        self.scratch = torch.empty((lib.cf2_ppo_scratch_bytes(max(m, n), d) + 7) // 8, dtype=torch.float64, device=gpu)
        self.grad = torch.full_like(self.flat, float("nan"))


def check_against_fp64(kernel_grads, kernel_summary, d, m, which, gpu, label, adv=None):
    g64, s64, _ = reference(d, m, which, torch.float64, "cpu", adv)
    g32, s32, _ = reference(d, m, which, torch.float32, gpu, adv)
    ek, e32 = rel_err(kernel_grads, g64), rel_err(g32, g64)
    print(f"{label} d={d} m={m}: kernel {max(ek):.3e} torch-fp32 {max(e32):.3e} per tensor "
          f"{['%.2e' % x for x in ek]} vs {['%.2e' % x for x in e32]}")
    for i, (a, b) in enumerate(zip(ek, e32)):
        assert a <= max(8.0 * b, FLOOR), (label, d, m, i, a, b)
    ks = kernel_summary.tolist()
    assert ks[0] == float(m) and all(v == 0.0 for v in ks[len(s64):])
    for i in range(1, len(s64)):
        den = abs(s64[i])
        a = abs(ks[i] - s64[i]) / den if den > 0 else abs(ks[i])
        b = abs(s32[i] - s64[i]) / den if den > 0 else abs(s32[i])
        print(f"   summary[{i}] kernel {a:.3e} torch-fp32 {b:.3e}")
        assert a <= max(8.0 * b, FLOOR), (label, "summary", d, m, i, ks[i], s64[i], s32[i])


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_ppo_entry_points(lib):
    from cf2sim._native import EXPORTED_SYMBOLS
    txt = open(os.path.join(ROOT, "include", "cf2sim.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(cf2_\w+)\s*\(", txt, flags=re.M))
    for name in NAMES:
        assert name in declared and name in EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.cf2_abi_version() == 8                       # additive change
    assert lib.cf2_ppo_scratch_bytes(1000, 35) == 0
    for d in (34, 42):
        assert lib.cf2_ppo_scratch_bytes(1, d) > 0 and lib.cf2_ppo_scratch_bytes(2 ** 32 - 1, d) % 8 == 0


def test_host_error_paths_need_no_device(lib):
    host = (ctypes.c_double * 64)()                         # never dereferenced: every call returns first
    p = ctypes.addressof(host)
    p += -p % 16
    pol = lambda **kw: lib.cf2_ppo_policy_grad(*[kw.get(k, v) for k, v in (
        ("w", p), ("d", 34), ("obs", p), ("act", p), ("lp", p), ("adv", p), ("n", 8), ("idx", None), ("m", 8), ("mom", None),
        ("clip", 0.2), ("mu_old", None), ("mu_out", None), ("logp_out", None), ("grad", None), ("summary", p),
        ("scratch", p), ("stream", None))])
    val = lambda **kw: lib.cf2_ppo_value_grad(*[kw.get(k, v) for k, v in (
        ("w", p), ("d", 34), ("obs", p), ("target", p), ("n", 8), ("idx", None), ("m", 8), ("val_out", None), ("grad", None),
        ("summary", p), ("scratch", p), ("stream", None))])
    for k in ("w", "obs", "act", "lp", "adv", "summary", "scratch"):
        assert pol(**{k: None}) == -1, k
    for k in ("w", "obs", "target", "summary", "scratch"):
        assert val(**{k: None}) == -1, k
    assert pol(d=35) == -4 and val(d=35) == -4
    assert pol(act=p + 8) == -1 and pol(obs=p + 4) == -1 and val(obs=p + 4) == -1 and pol(summary=p + 4) == -1
    assert pol(m=9) == -1 and val(m=9) == -1                # m > n without idx
    assert pol(m=0) == 0 and val(m=0) == 0
    assert pol(m=0, w=None) == 0


@pytest.mark.parametrize("d", [34, 42])
def test_scatter_flat_grad_inverts_the_pack(d):
    from cf2sim.ppo import flat_slice, scatter_flat_grad
    from cf2sim.rollout import MLPActorCritic, pack_policy_weights
    ac = MLPActorCritic(obs_dim=d)
    count = pack_policy_weights(ac).numel()
    g = torch.randn(count, generator=torch.Generator().manual_seed(d))
    S = sizes(d)
    assert flat_slice(ac, "pi") == (0, S["pi_end"]) and flat_slice(ac, "v") == (S["v_begin"], S["v_end"])
    scatter_flat_grad(ac, g, "pi")
    assert all(p.grad is None for p in ac.v_net.parameters())
    scatter_flat_grad(ac, g, "v")
    twin = MLPActorCritic(obs_dim=d)
    with torch.no_grad():
        for p, q in zip(list(twin.pi_net.parameters()) + list(twin.v_net.parameters()),
                        list(ac.pi_net.parameters()) + list(ac.v_net.parameters())):
            p.copy_(q.grad)
    back = pack_policy_weights(twin)
    assert torch.equal(back[:S["pi_end"]], g[:S["pi_end"]])
    assert torch.equal(back[S["v_begin"]:S["v_end"]], g[S["v_begin"]:S["v_end"]])


def test_torch_losses_agree_with_central_differences():
    from cf2sim.ppo import policy_loss_torch, value_loss_torch
    P = pool(34)
    m = 64
    ac = copy.deepcopy(P["ac"]).double()
    obs, act, lpo, adv, tgt = (P[k][:m].double() for k in ("obs", "act", "logp_old", "adv", "target"))
    for which, loss in (("pi", lambda: policy_loss_torch(ac, obs, act, lpo, adv, CLIP)),
                        ("v", lambda: value_loss_torch(ac, obs, tgt))):
        for p in ac.parameters():
            p.grad = None
        loss().backward()
        net = ac.pi_net if which == "pi" else ac.v_net
        scale = max(float(p.grad.abs().max()) for p in net.parameters())
        for p, index in ((net[0].weight, (3, 5)), (net[0].bias, (7,)), (net[2].weight, (11, 2)), (net[4].weight, (0, 9)),
                         (net[4].bias, (0,))):
            h = 1e-6
            with torch.no_grad():
                old = float(p[index])
                p[index] = old + h
                up = float(loss())
                p[index] = old - h
                down = float(loss())
                p[index] = old
            fd = (up - down) / (2 * h)
            # the rows are 1e-4 / 1e-5 away from the kinks, so the loss is smooth over +-h; the
            # central difference's own error is h^2 f''' / 6 plus the loss's rounding / h
            assert abs(fd - float(p.grad[index])) <= 1e-7 * scale + 1e-9, (which, index, fd, float(p.grad[index]))


def test_pool_covers_the_cases():
    for d in (34, 42):
        P = pool(d)
        assert P["dropped"] <= 0.01, P["dropped"]
        for m in (1000, POOL):
            c, pos = P["clipped"][:m], P["pos"][:m]
            for case in (c & pos, c & ~pos, ~c & pos, ~c & ~pos):
                assert float(case.double().mean()) >= 0.05
        assert not bool(P["clipped"][0])           # m = 1: a row with a gradient


def synthetic_rollout(seed, T=6, N=40, d=34):
    from cf2sim.rollout import Rollout
    g = torch.Generator().manual_seed(seed)
    ac = make_ac(d, seed)
    obs = ac.obs_oms.mean + ac.obs_oms.std * torch.randn(T, N, d, generator=g)
    with torch.no_grad():
        act, val, logp = ac.step(obs.view(-1, d), generator=g)
    z = torch.zeros(T, N)
    adv = torch.randn(T, N, generator=g) * 3.0 + 1.0
    ret = torch.randn(T, N, generator=g)
    ro = Rollout(obs, act.view(T, N, 4), z, val.view(T, N), logp.view(T, N), z.bool(), z.bool(), adv, ret, obs[0],
                 z[0], z, z)
    return ac, ro


def test_updater_torch_path_on_a_synthetic_rollout():
    from cf2sim.ppo import PPOUpdater
    ac, ro = synthetic_rollout(3)
    mk = lambda **kw: PPOUpdater(ac, torch.optim.Adam(ac.pi_net.parameters(), lr=3e-4),
                                 torch.optim.Adam(ac.v_net.parameters(), lr=1e-3), CLIP, device=False,
                                 generator=torch.Generator().manual_seed(1), **kw)
    up = mk(target_kl=1e9, train_pi_iterations=4, train_v_iterations=1)
    first = up.update(ro)
    second = up.update(ro)
    assert first["StopIter"] == 4 and set(first) == {"LossPi", "LossV", "KL", "StopIter", "ClipFrac"}
    assert second["LossV"] < first["LossV"]                 # one pass of 16 mini-batch steps lowered it
    assert first["KL"] > 0.0 and 0.0 <= first["ClipFrac"] <= 1.0
    # the first iteration starts at ratio = 1 up to the rounding of logp: LossPi = -mean(A) of the
    # standardised advantages = 0
    assert abs(first["LossPi"]) < 1e-5
    assert mk(target_kl=1e-12, train_pi_iterations=80, train_v_iterations=0).update(ro)["StopIter"] == 1
    for n in (240, 250, 7):
        mbs = up.value_minibatches(n, torch.device("cpu"))
        assert len(mbs) == min(16, n) and max(len(b) for b in mbs) - min(len(b) for b in mbs) <= 1
        assert torch.equal(torch.cat(mbs).sort().values, torch.arange(n))
    # the rows the value passes read: every row once per pass
    seen = []
    import cf2sim.ppo as ppo
    orig = ppo.value_loss_torch
    try:
        ppo.value_loss_torch = lambda a, o, t: (seen.append(o), orig(a, o, t))[1]
        mk(target_kl=1e9, train_pi_iterations=0, train_v_iterations=2).update(ro)
    finally:
        ppo.value_loss_torch = orig
    rows = ro.obs.reshape(-1, 34)
    assert len(seen) == 1 + 2 * 16                          # the `before` loss, then 2 passes
    for k in range(2):
        used = torch.cat(seen[1 + 16 * k:1 + 16 * (k + 1)])
        assert used.shape == rows.shape
        assert torch.equal(used[used[:, 0].argsort()], rows[rows[:, 0].argsort()])


# ---------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_paths_launch_nothing(gpu, lib):
    B = Dev(lib, gpu, 34, 64)
    grad = torch.full_like(B.flat, 7.0)
    mu_out = torch.full((64, 4), 7.0, device=gpu)
    lp_out = torch.full((64,), 7.0, device=gpu)
    pad = torch.zeros(64 * 4 + 4, device=gpu)
    act_bad = pad[1:1 + 64 * 4]                              # 4 bytes off a 16-byte boundary
    assert act_bad.data_ptr() % 16 == 4
    p = lambda t: None if t is None else t.data_ptr()

    def pol(w=B.flat, d=34, obs=B.obs, act=B.act, n=64, m=64, summary=B.summary):
        return lib.cf2_ppo_policy_grad(p(w), d, p(obs), p(act), p(B.logp_old), p(B.adv), n, None, m, None, CLIP, None,
                                       p(mu_out), p(lp_out), p(grad), p(summary), p(B.scratch), None)

    def val(w=B.flat, d=34, obs=B.obs, n=64, m=64, summary=B.summary):
        return lib.cf2_ppo_value_grad(p(w), d, p(obs), p(B.target), n, None, m, p(lp_out), p(grad), p(summary),
                                      p(B.scratch), None)

    assert pol(w=None) == -1 and pol(obs=None) == -1 and pol(summary=None) == -1 and val(w=None) == -1
    assert pol(d=35) == -4 and val(d=35) == -4
    assert pol(act=act_bad) == -1
    assert pol(n=63) == -1 and val(n=63) == -1              # m > n without idx
    assert pol(m=0) == 0 and val(m=0) == 0
    torch.cuda.synchronize()
    for t in (grad, mu_out, lp_out, B.summary):
        assert bool((t == 7.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("d", [34, 42])
def test_policy_gradient_and_summary_against_fp64(gpu, lib, d, m):
    from cf2sim.ppo import policy_grad_device
    B = Dev(lib, gpu, d, m)
    policy_grad_device(B.flat, B.obs, B.act, B.logp_old, B.adv, CLIP, B.summary, B.scratch, grad=B.grad, mu_old=B.mu_old)
    check_against_fp64(flat_to_tensors(B.grad, d, "pi"), B.summary, d, m, "pi", gpu, "policy")


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("d", [34, 42])
def test_value_gradient_and_summary_against_fp64(gpu, lib, d, m):
    from cf2sim.ppo import value_grad_device
    B = Dev(lib, gpu, d, m)
    value_grad_device(B.flat, B.obs, B.target, B.summary, B.scratch, grad=B.grad)
    check_against_fp64(flat_to_tensors(B.grad, d, "v"), B.summary, d, m, "v", gpu, "value")


@pytest.mark.gpu
def test_index_subset_is_the_dense_call_on_the_gathered_rows(gpu, lib):
    from cf2sim.ppo import policy_grad_device, value_grad_device
    d, n, m = 34, 5000, 1000
    B = Dev(lib, gpu, d, m, n=n)
    g = torch.Generator().manual_seed(8)
    idx = torch.randint(0, n, (m,), generator=g)
    idx[100:150] = idx[0:50]                                 # repeats
    idx[-1] = n - 1
    idx_d = idx.to(gpu, dtype=torch.int32)
    sel = idx.to(gpu)
    res = []
    for gathered in (False, True):
        obs, act, lpo, adv, tgt = ((t[sel].contiguous() if gathered else t) for t in (B.obs, B.act, B.logp_old, B.adv,
                                                                                      B.target))
        kw = {} if gathered else {"idx": idx_d}
        gp, gv = torch.full_like(B.flat, float("nan")), torch.full_like(B.flat, float("nan"))
        sp, sv = B.summary.clone(), B.summary.clone()
        mu, lp, v = torch.empty(m, 4, device=gpu), torch.empty(m, device=gpu), torch.empty(m, device=gpu)
        policy_grad_device(B.flat, obs, act, lpo, adv, CLIP, sp, B.scratch, grad=gp, mu_out=mu, logp_out=lp, **kw)
        value_grad_device(B.flat, obs, tgt, sv, B.scratch, grad=gv, val_out=v, **kw)
        res.append((gp, gv, sp, sv, mu, lp, v))
    S = sizes(d)
    for a, b in zip(*res):
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
    assert not bool(torch.isnan(res[0][0][:S["pi_end"]]).any()) and not bool(torch.isnan(res[0][2]).any())


@pytest.mark.gpu
def test_advantage_moments_standardise_on_the_fly(gpu, lib):
    from cf2sim.ppo import policy_grad_device
    d, m = 34, 1000
    B = Dev(lib, gpu, d, m)
    adv = (B.adv * 3.0 + 1.5).contiguous()
    mom = torch.empty(2, dtype=torch.float64, device=gpu)
    cm = torch.empty(lib.cf2_column_moments_scratch_bytes(m, 1) // 8 + 1, dtype=torch.float64, device=gpu)
    assert lib.cf2_column_moments(adv.data_ptr(), m, 1, mom.data_ptr(), cm.data_ptr(), None) == 0
    policy_grad_device(B.flat, B.obs, B.act, B.logp_old, adv, CLIP, B.summary, B.scratch, grad=B.grad, adv_moments=mom,
                       mu_old=B.mu_old)
    a64 = adv.double().cpu()
    std = torch.sqrt(((a64 - a64.mean()) ** 2).sum() / m)
    check_against_fp64(flat_to_tensors(B.grad, d, "pi"), B.summary, d, m, "pi", gpu, "moments",
                       adv=(a64 - a64.mean()) / (std + 1e-8))


@pytest.mark.gpu
def test_evaluate_only_gives_the_same_summary_bits(gpu, lib):
    from cf2sim.ppo import policy_grad_device, value_grad_device
    from cf2sim.rollout import FusedActorCritic
    d, m = 34, 1000
    B = Dev(lib, gpu, d, m)
    runs = []
    for grad in (B.grad, None, None):
        sp, sv = B.summary.clone(), B.summary.clone()
        mu, lp, v = torch.empty(m, 4, device=gpu), torch.empty(m, device=gpu), torch.empty(m, device=gpu)
        policy_grad_device(B.flat, B.obs, B.act, B.logp_old, B.adv, CLIP, sp, B.scratch, grad=grad, mu_old=B.mu_old,
                           mu_out=mu, logp_out=lp)
        value_grad_device(B.flat, B.obs, B.target, sv, B.scratch, grad=grad, val_out=v)
        runs.append((sp, sv, mu, lp, v))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    again = torch.full_like(B.flat, float("nan"))
    policy_grad_device(B.flat, B.obs, B.act, B.logp_old, B.adv, CLIP, B.summary, B.scratch, grad=again, mu_old=B.mu_old)
    value_grad_device(B.flat, B.obs, B.target, B.summary, B.scratch, grad=again)
    S = sizes(d)
    assert torch.equal(again[:S["pi_end"]], B.grad[:S["pi_end"]])
    assert torch.equal(again[S["v_begin"]:S["v_end"]], B.grad[S["v_begin"]:S["v_end"]])
    # mu and V against the collect path's forward in fp32 mode
    fused = FusedActorCritic(copy.deepcopy(pool(d)["ac"]).to(gpu), precision="fp32")
    mu_f, val_f, _ = fused.step(B.obs, deterministic=True)
    mu, v = runs[0][2], runs[0][4]
    assert float((mu - mu_f).abs().max()) <= 1e-5 * float(mu_f.abs().max())
    assert float((v - val_f).abs().max()) <= 1e-5 * float(val_f.abs().max())
    _, _, ex = reference(d, m, "pi", torch.float64, "cpu")
    assert float((runs[0][3].double().cpu() - ex["logp"]).abs().max()) <= 1e-5 * float(ex["logp"].abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("d", [34, 42])
def test_each_call_writes_exactly_its_slice(gpu, lib, d):
    from cf2sim.ppo import policy_grad_device, value_grad_device
    B = Dev(lib, gpu, d, 100)
    S = sizes(d)
    pattern = torch.full_like(B.flat, float("nan"))
    policy_grad_device(B.flat, B.obs, B.act, B.logp_old, B.adv, CLIP, B.summary, B.scratch, grad=B.grad)
    nan = torch.isnan(B.grad)
    assert not bool(nan[:S["pi_end"]].any()) and bool(nan[S["pi_end"]:].all())
    assert torch.equal(B.grad[S["pi_end"]:].view(torch.int32), pattern[S["pi_end"]:].view(torch.int32))
    gv = pattern.clone()
    value_grad_device(B.flat, B.obs, B.target, B.summary, B.scratch, grad=gv)
    nan = torch.isnan(gv)
    assert not bool(nan[S["v_begin"]:S["v_end"]].any())
    assert bool(nan[:S["v_begin"]].all()) and bool(nan[S["v_end"]:].all())
    assert gv.numel() == S["v_end"] + 2 * d


@pytest.mark.gpu
def test_updater_device_path_follows_the_torch_path(gpu):
    """End to end: collect N = 256, T = 8, then PPOUpdater with device=True and device=False from
    identical copies, SGD, 3 policy iterations, 1 value pass, the same permutations.  With SGD the
    parameter difference is lr x the sum of the gradient differences.  Each gradient pair differs by
    at most (max(8 e32, 2^-20) + e32) |g|_inf per tensor -- the kernel's bound plus torch-fp32's own
    error e32, both against fp64 -- so the parameters agree within lr x steps x that, with e32 and
    |g|_inf measured on fp64 autograd at the start (policy: the full batch, 3 steps; value: the
    largest over the 16 mini-batches, 16 steps).  Each step also rounds p - lr g into the fp32
    parameter on both paths, and two values that close may round to neighbouring floats: one ulp,
    at most 2^-23 |p|_inf, per step on top.  Measured on an MI355X: the policy tensors differ by
    0 .. 1.5e-8 (one ulp of a weight in [0.125, 0.25)) against gradient terms of 4e-10 .. 7e-9, the
    value tensors by 3e-8 .. 2.4e-7 against gradient terms of 8e-7 .. 8e-6."""
    from cf2sim.ppo import PPOUpdater, policy_loss_torch, value_loss_torch
    from cf2sim.rollout import FusedActorCritic, MLPActorCritic, collect
    from cf2sim.vec_env import BatchedCrazyflieEnv
    n_env, T, lr = 256, 8, 1e-2
    envs = BatchedCrazyflieEnv(ENV_ID, n_env, seed=21, want_final_obs=True)
    torch.manual_seed(5)
    ac_d = MLPActorCritic().to(gpu)
    with torch.no_grad():
        ac_d.obs_oms.mean.normal_(0.0, 0.1)
        ac_d.obs_oms.std.uniform_(0.5, 1.5)
    fused = FusedActorCritic(ac_d, seed=2)
    ro = collect(envs, fused, T)
    ac_t = copy.deepcopy(ac_d)
    rows = lambda t, *s: t.reshape(-1, *s)
    obs, act, lpo, ret = rows(ro.obs, 34), rows(ro.act, 4), rows(ro.logp), rows(ro.ret)
    a64 = rows(ro.adv).double()
    adv = ((a64 - a64.mean()) / (torch.sqrt(((a64 - a64.mean()) ** 2).mean()) + 1e-8))

    def grads_of(dtype, which, sel=slice(None)):
        ac = copy.deepcopy(ac_t).to(dtype)
        c = lambda t: t[sel].to(dtype)
        loss = policy_loss_torch(ac, c(obs), c(act), c(lpo), c(adv), CLIP) if which == "pi" \
            else value_loss_torch(ac, c(obs), c(ret))
        loss.backward()
        return module_grads(ac, which)

    def budget(which, sels, steps):
        tol, gmax = [0.0] * 6, [0.0] * 6
        for sel in sels:
            g64, g32 = grads_of(torch.float64, which, sel), grads_of(torch.float32, which, sel)
            for i, e in enumerate(rel_err(g32, g64)):
                tol[i] = max(tol[i], max(8.0 * e, FLOOR) + e)
                gmax[i] = max(gmax[i], float(g64[i].abs().max()))
        return [lr * steps * t * g for t, g in zip(tol, gmax)]

    mk = lambda ac, dev, fu: PPOUpdater(ac, torch.optim.SGD(ac.pi_net.parameters(), lr=lr),
                                        torch.optim.SGD(ac.v_net.parameters(), lr=lr), CLIP, 1e9, train_pi_iterations=3,
                                        train_v_iterations=1, fused=fu, device=dev,
                                        generator=torch.Generator().manual_seed(17))
    mbs = mk(ac_t, False, None).value_minibatches(obs.shape[0], gpu)       # the permutation both runs draw
    bound = {"pi": budget("pi", [slice(None)], 3), "v": budget("v", mbs, len(mbs))}
    out_d = mk(ac_d, True, fused).update(ro)
    out_t = mk(ac_t, False, None).update(ro)
    assert out_d["StopIter"] == out_t["StopIter"] == 3
    for k in ("LossPi", "LossV", "KL", "ClipFrac"):
        print(k, out_d[k], out_t[k])
        assert abs(out_d[k] - out_t[k]) <= 1e-4 * max(abs(out_t[k]), 1e-3), k
    for which in ("pi", "v"):
        nets = [(ac_d.pi_net, ac_t.pi_net), (ac_d.v_net, ac_t.v_net)][which == "v"]
        params = [[p for m in net if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)] for net in nets]
        steps = 3 if which == "pi" else len(mbs)
        for i, (p, q) in enumerate(zip(*params)):
            diff = float((p.detach() - q.detach()).abs().max())
            limit = bound[which][i] + steps * 2.0 ** -23 * float(q.detach().abs().max())
            print(f"{which}[{i}] diff {diff:.3e} gradient term {bound[which][i]:.3e} limit {limit:.3e}")
            assert diff <= limit, (which, i, diff, limit)
    # the fused forward was re-packed by update(); the next collect runs on the new weights
    ro2 = collect(envs, fused, T, obs=ro.last_obs, out=ro)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ro2.obs).all()) and bool(torch.isfinite(ro2.adv).all())
