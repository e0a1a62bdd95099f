"""The PPO update resident on the GPU: cf2_adam_step (csrc/cf2sim_optim.hip), cf2_ppo_policy_grad_gated
(csrc/cf2sim_ppo.hip) and, in cf2sim, unpack_policy_weights, FusedActorCritic.sync_from_flat,
adam_step_device, DeviceAdam and ResidentPPOUpdater.

Adam.  The reference is the formula of include/cf2sim.h in fp64 on the CPU (state and weights in fp64
through all 20 steps), the yardstick torch.optim.Adam(foreach=False) in fp32 on the same gradients,
after torch.nn.utils.clip_grad_norm_ where clipping is on.  All three get the hyper-parameters as the
fp32 values the C call receives (the ABI passes floats: 0.999f is 0.99900001287...; with the decimal
value the fp64 reference and torch would differ from the kernel by 1 - beta2's relative rounding,
4.7e-5, which says nothing about the kernel).  Per slice and per array (w, m, v) the error is
|got - want|_inf / |want|_inf; the kernel may be at most 8 x torch-fp32's error, with a floor of 2^-20,
the rule of tests/test_ppo_update.py.  The kernel evaluates every word's update in fp64 and rounds
once, so it is expected to sit below torch.  Gradients: fresh randn per step, every second step scaled
by 0.1; with max_grad_norm = half the median of the 20 norms the large steps clip and the small ones
do not (``test_adam_inputs_clip_some_steps`` checks that without a GPU).

The resident update is compared bit for bit with the reference's loop written out in the test from
the same kernels (two passes over the rows per iteration, a host read and ``break`` per iteration).
That rests on evaluate-only and gradient calls giving the same summary bits
(tests/test_ppo_update.py::test_evaluate_only_gives_the_same_summary_bits).  Case (c)'s learning rate
and KL target were picked on the CPU with PPOUpdater(device=False) and torch.optim.Adam on this
synthetic rollout (the table is at PI_LR_C below).
"""
import copy
import ctypes
import functools
import math
import os
import re
import statistics

import pytest
import torch

from test_ppo_update import CLIP, ENV_ID, FLOOR, Dev, sizes, synthetic_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cf2_adam_step", "cf2_ppo_policy_grad_gated")
STEPS = 20
f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
LR, B1, B2, EPS = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8)
V42 = (sizes(42)["v_begin"], sizes(42)["v_end"] - sizes(42)["v_begin"])
SLICES = ((0, 1), (3, 63), (17, 1025), V42)
WORDS = sizes(42)["v_end"] + 2 * 42                       # the flat block of obs_dim 42
# case (c) of the resident update: the KL after steps 1..8 of PPOUpdater(device=False) on the CPU with
# torch.optim.Adam(lr=PI_LR_C) behind clip_grad_norm_(MAX_NORM) on synthetic_rollout(11, T=8, N=515, d):
#   d = 34   8.40e-5  3.35e-4  7.51e-4  1.33e-3  2.03e-3  2.74e-3  3.39e-3  3.91e-3
#   d = 42   6.63e-5  2.65e-4  5.96e-4  1.06e-3  1.65e-3  2.36e-3  3.09e-3  3.74e-3
# The target lies between steps 4 and 5 of both, at least 9 % from either: the loop stops after step 5.
# Pre-clip policy gradient norms there: 0.144 0.145 0.144 0.145 0.130 0.111 0.108 0.105 ..., so
# MAX_NORM clips the first steps and not the later ones of case (a).
PI_LR_C, TARGET_KL_C, MAX_NORM = 3e-4, 1.5e-3, 0.12


@pytest.fixture(scope="module")
def lib():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    return _native.load()


# ---------------------------------------------------------------------------------------------
# Adam: inputs and references, built once per (slice, clipping) on the CPU
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adam_case(begin, count, clip):
    g = torch.Generator().manual_seed(1000 + begin + count)
    w0 = torch.randn(WORDS, generator=g) * 0.3
    grads = torch.randn(STEPS, WORDS, generator=g) * 0.05
    grads[1::2] *= 0.1
    sl = slice(begin, begin + count)
    norms = [math.sqrt(float((grads[t, sl].double() ** 2).sum())) for t in range(STEPS)]
    max_norm = f32(0.5 * statistics.median(norms)) if clip else 0.0
    # fp64 reference: the header's formula
    w, m, v = w0[sl].double(), torch.zeros(count, dtype=torch.float64), torch.zeros(count, dtype=torch.float64)
    for t in range(1, STEPS + 1):
        gt = grads[t - 1, sl].double()
        if max_norm > 0:
            gt = gt * min(1.0, max_norm / (norms[t - 1] + 1e-6))
        m = B1 * m + (1.0 - B1) * gt
        v = B2 * v + (1.0 - B2) * gt * gt
        w = w - LR / (1.0 - B1 ** t) * m / (v.sqrt() / math.sqrt(1.0 - B2 ** t) + EPS)
    # the yardstick: torch's fp32 Adam
    p = torch.nn.Parameter(w0[sl].clone())
    opt = torch.optim.Adam([p], lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
    for t in range(STEPS):
        p.grad = grads[t, sl].clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
    st = opt.state[p]
    return {"w0": w0, "grads": grads, "norms": norms, "max_norm": max_norm, "want": (w, m, v),
            "torch": (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())}


def err(got, want):
    den = float(want.abs().max())
    num = float((got.double().cpu() - want).abs().max())
    return num / den if den > 0 else (0.0 if num == 0 else math.inf)


def run_adam(gpu, begin, count, clip):
    """20 kernel steps on canaried blocks; returns the blocks, the step word and the norms."""
    from cf2sim.ppo import adam_step_device
    C = adam_case(begin, count, clip)
    sl = slice(begin, begin + count)
    nan = torch.full((WORDS,), float("nan"))
    w, m, v = nan.clone(), nan.clone(), nan.clone()
    w[sl], m[sl], v[sl] = C["w0"][sl], 0.0, 0.0
    w, m, v, grads = w.to(gpu), m.to(gpu), v.to(gpu), C["grads"].to(gpu)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    norm = torch.zeros(1, dtype=torch.float64, device=gpu)
    norms = []
    for t in range(STEPS):
        adam_step_device(w, grads[t], m, v, begin, count, step, LR, B1, B2, EPS, C["max_norm"], norm_out=norm)
        norms.append(norm.clone())
    return w, m, v, step, torch.cat(norms), grads


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_resident_entry_points(lib):
    from cf2sim._native import EXPORTED_SYMBOLS
    txt = open(os.path.join(ROOT, "include", "cf2sim.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(cf2_\w+)\s*\(", txt, flags=re.M))
    out = os.popen(f"nm -D --defined-only {lib._name}").read()
    for name in NAMES:
        assert name in declared and name in EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported"
    assert lib.cf2_abi_version() == 8                       # additive change


def test_host_error_paths_need_no_device(lib):
    host = (ctypes.c_double * 64)()                         # never dereferenced: every call returns first
    p = ctypes.addressof(host)
    p += -p % 16
    adam = lambda **kw: lib.cf2_adam_step(*[kw.get(k, v) for k, v in (
        ("w", p), ("grad", p), ("m", p), ("v", p), ("begin", 0), ("count", 8), ("step", p), ("lr", 1e-3), ("b1", 0.9),
        ("b2", 0.999), ("eps", 1e-8), ("max_norm", 0.0), ("norm_out", None), ("kl", None), ("target_kl", 0.0),
        ("ctrl", None), ("stream", None))])
    for k in ("w", "grad", "m", "v", "step"):
        assert adam(**{k: None}) == -1, k
    for k in ("w", "grad", "m", "v", "step", "ctrl"):
        assert adam(**{k: p + 2}) == -1, k
    for k in ("norm_out", "kl"):
        assert adam(**{k: p + 4}) == -1, k
    assert adam(begin=2 ** 32 - 4, count=8) == -1           # begin + count past 32 bits
    assert adam(lr=-1e-3) == -1 and adam(lr=float("nan")) == -1 and adam(lr=float("inf")) == -1
    assert adam(count=(1 << 20) + 1) == -4
    assert adam(count=0) == 0 and adam(count=0, w=None) == 0
    gated = lambda **kw: lib.cf2_ppo_policy_grad_gated(*[kw.get(k, v) for k, v in (
        ("w", p), ("d", 34), ("obs", p), ("act", p), ("lp", p), ("adv", p), ("n", 8), ("idx", None), ("m", 8), ("mom", None),
        ("clip", 0.2), ("mu_old", None), ("mu_out", None), ("logp_out", None), ("grad", None), ("summary", p),
        ("scratch", p), ("ctrl", p), ("stream", None))])
    assert gated(d=35) == -4
    assert gated(w=None) == -1 and gated(ctrl=p + 2) == -1 and gated(m=9) == -1
    assert gated(m=0) == 0


@pytest.mark.parametrize("d", [34, 42])
def test_unpack_inverts_the_pack(d):
    from cf2sim.rollout import MLPActorCritic, pack_policy_weights, unpack_policy_weights
    torch.manual_seed(d)
    ac1, ac2 = MLPActorCritic(obs_dim=d), MLPActorCritic(obs_dim=d)
    with torch.no_grad():
        ac2.log_std.fill_(-1.25)
        ac2.obs_oms.mean.normal_()
        ac2.obs_oms.std.uniform_(0.5, 2.0)
    keep = [t.clone() for t in (ac2.log_std, ac2.obs_oms.mean, ac2.obs_oms.std, ac2.obs_oms.count)]
    linears = lambda ac: [p for net in (ac.pi_net, ac.v_net) for m in net if isinstance(m, torch.nn.Linear)
                          for p in (m.weight, m.bias)]
    assert not any(torch.equal(a, b) for a, b in zip(linears(ac1), linears(ac2)) if a.dim() == 2)
    unpack_policy_weights(ac2, pack_policy_weights(ac1))
    assert len(linears(ac1)) == 12
    for a, b in zip(linears(ac1), linears(ac2)):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
    for a, b in zip(keep, (ac2.log_std, ac2.obs_oms.mean, ac2.obs_oms.std, ac2.obs_oms.count)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        unpack_policy_weights(ac2, pack_policy_weights(ac1)[:-1])


@pytest.mark.parametrize("begin,count", SLICES)
def test_adam_inputs_clip_some_steps(begin, count):
    C = adam_case(begin, count, True)
    clipped = [n + 1e-6 > C["max_norm"] for n in C["norms"]]
    assert C["max_norm"] > 0 and any(clipped) and not all(clipped), (C["max_norm"], C["norms"])
    assert adam_case(begin, count, False)["max_norm"] == 0.0
    for got, want in zip(C["torch"], C["want"]):             # the yardstick itself follows the formula
        assert err(got, want) < 1e-4


# ---------------------------------------------------------------------------------------------
# on the GPU: cf2_adam_step
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("begin,count", SLICES)
def test_adam_against_fp64(gpu, lib, begin, count, clip):
    C = adam_case(begin, count, clip)
    w, m, v, step, norms, grads = run_adam(gpu, begin, count, clip)
    sl = slice(begin, begin + count)
    for name, got, want, ref32 in zip("wmv", (w, m, v), C["want"], C["torch"]):
        ek, e32 = err(got[sl], want), err(ref32, want)
        print(f"adam [{begin}, {begin + count}) clip={clip} {name}: kernel {ek:.3e} torch-fp32 {e32:.3e}")
        assert ek <= max(8.0 * e32, FLOOR), (name, begin, count, clip, ek, e32)
    for t, n in enumerate(norms.tolist()):
        assert abs(n - C["norms"][t]) <= 2.0 ** -40 * C["norms"][t], (t, n, C["norms"][t])
    assert int(step.item()) == STEPS
    outside = torch.ones(WORDS, dtype=torch.bool)
    outside[sl] = False
    for t in (w, m, v):                                      # the canaries: every word outside the slice
        assert bool(torch.isnan(t.cpu()[outside]).all()) and not bool(torch.isnan(t.cpu()[sl]).any())
    assert torch.equal(grads.cpu().view(torch.int32), C["grads"].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("begin,count", SLICES)
def test_adam_gives_the_same_bits_twice(gpu, lib, begin, count):
    a, b = run_adam(gpu, begin, count, True), run_adam(gpu, begin, count, True)
    sl = slice(begin, begin + count)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x[sl].view(torch.int32), y[sl].view(torch.int32))
    assert torch.equal(a[4].view(torch.int64), b[4].view(torch.int64))


@pytest.mark.gpu
def test_adam_gate(gpu, lib):
    from cf2sim.ppo import adam_step_device
    begin, count = 3, 63
    C = adam_case(begin, count, False)
    target = 0.0123
    t32 = f32(target)                                        # what the call compares with

    def run(ctrl0, kl):
        w = C["w0"].to(gpu)
        m, v = torch.full_like(w, 0.25), torch.full_like(w, 0.5)
        step = torch.full((1,), 5, dtype=torch.int32, device=gpu)
        norm = torch.full((1,), -1.0, dtype=torch.float64, device=gpu)
        ctrl = torch.tensor([ctrl0, 0, 0, 0], dtype=torch.int32, device=gpu)
        summ = torch.tensor([1.0, 2.0, 3.0, 4.0, kl, 6.0, 0.0, 0.0], dtype=torch.float64, device=gpu)
        before = [t.clone() for t in (w, m, v, step, norm, summ)]
        adam_step_device(w, C["grads"][0].to(gpu), m, v, begin, count, step, LR, B1, B2, EPS, 0.0, norm_out=norm,
                         kl_summary=summ, target_kl=target, ctrl=ctrl)
        raw = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)      # a NaN equals itself
        same = [torch.equal(raw(a), raw(b)) for a, b in zip(before, (w, m, v, step, norm, summ))]
        return same, ctrl.tolist(), int(step.item())

    same, ctrl, step = run(1, 0.0)                           # already stopped
    assert all(same) and ctrl == [1, 0, 0, 0] and step == 5
    same, ctrl, step = run(0, t32)                           # KL == target: strict comparison, step taken
    assert same == [False, False, False, False, False, True] and ctrl == [0, 1, 0, 0] and step == 6
    same, ctrl, step = run(0, math.nextafter(t32, math.inf))
    assert all(same) and ctrl == [1, 0, 0, 0] and step == 5
    same, ctrl, step = run(0, float("nan"))                  # NaN compares false: step taken, as the reference
    assert same == [False, False, False, False, False, True] and ctrl == [0, 1, 0, 0] and step == 6


@pytest.mark.gpu
def test_adam_wrapper_rejects_a_slice_outside_the_block(gpu, lib):
    from cf2sim.ppo import DeviceAdam, adam_step_device
    w = torch.zeros(100, device=gpu)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError):
        adam_step_device(w, w.clone(), w.clone(), w.clone(), 90, 11, step, 1e-3)
    with pytest.raises(ValueError):
        adam_step_device(w, w.clone()[:99], w.clone(), w.clone(), 0, 10, step, 1e-3)
    with pytest.raises(ValueError):
        DeviceAdam(100, 90, 11, 1e-3, device=gpu)
    assert int(step.item()) == 0 and not bool(w.any())


# ---------------------------------------------------------------------------------------------
# on the GPU: the gated gradient call
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", [34, 42])
def test_gated_gradient_call(gpu, lib, d):
    from cf2sim.ppo import policy_grad_device
    m = 1000
    B = Dev(lib, gpu, d, m)

    def run(ctrl, scratch_fill=None):
        grad = torch.full_like(B.flat, float("nan"))
        summ = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        mu, lp = torch.full((m, 4), 7.0, device=gpu), torch.full((m,), 7.0, device=gpu)
        if scratch_fill is not None:
            B.scratch.fill_(scratch_fill)
        policy_grad_device(B.flat, B.obs, B.act, B.logp_old, B.adv, CLIP, summ, B.scratch, grad=grad, mu_old=B.mu_old,
                           mu_out=mu, logp_out=lp, ctrl=ctrl)
        return grad, summ, mu, lp

    bits = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    plain = run(None)
    open_ = run(torch.zeros(4, dtype=torch.int32, device=gpu))
    for a, b in zip(plain, open_):
        assert torch.equal(bits(a), bits(b))
    assert not bool(torch.isnan(plain[0][:sizes(d)["pi_end"]]).any()) and float(plain[1][0]) == m
    ctrl = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=gpu)
    grad, summ, mu, lp = run(ctrl, scratch_fill=-3.0)
    assert bool(torch.isnan(grad).all()) and bool((summ == 7.0).all()) and bool((mu == 7.0).all())
    assert bool((lp == 7.0).all()) and bool((B.scratch == -3.0).all()) and ctrl.tolist() == [1, 0, 0, 0]
    grad, summ, mu, lp = run(torch.tensor([5, 0, 0, 0], dtype=torch.int32, device=gpu))
    assert bool(torch.isnan(grad).all()) and bool((summ == 7.0).all())       # any non-zero word closes the gate


# ---------------------------------------------------------------------------------------------
# on the GPU: ResidentPPOUpdater
# ---------------------------------------------------------------------------------------------
def gpu_rollout(seed, gpu, T=8, N=515, d=34):
    import dataclasses
    from cf2sim.rollout import Rollout
    ac, ro = synthetic_rollout(seed, T=T, N=N, d=d)
    moved = {f.name: getattr(ro, f.name).to(gpu) for f in dataclasses.fields(ro) if f.name != "storage"}
    return ac.to(gpu), Rollout(**moved)


def literal_update(ac, ro, pi_lr, v_lr, target_kl, iters, v_iters, num_mb, generator, max_grad_norm=0.0):
    """The reference's loop, two passes over the rows per policy iteration and a host read after
    each, from the same kernels; fresh optimiser state.  Returns the flat block, the optimiser state
    and the log entries."""
    from cf2sim import _native
    from cf2sim.ppo import adam_step_device, flat_slice, policy_grad_device, value_grad_device
    from cf2sim.rollout import pack_policy_weights
    lib = _native.load()
    d = ro.obs.shape[-1]
    obs, act = ro.obs.reshape(-1, d).contiguous(), ro.act.reshape(-1, 4).contiguous()
    lpo, adv, ret = (t.reshape(-1).contiguous() for t in (ro.logp, ro.adv, ro.ret))
    n, dev = obs.shape[0], obs.device
    nbytes = max(lib.cf2_ppo_scratch_bytes(n, d), lib.cf2_column_moments_scratch_bytes(n, 1))
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    mom = torch.empty(2, dtype=torch.float64, device=dev)
    summary = torch.empty(8, dtype=torch.float64, device=dev)
    mu_old = torch.empty(n, 4, device=dev)
    assert lib.cf2_column_moments(adv.data_ptr(), n, 1, mom.data_ptr(), scratch.data_ptr(), None) == 0
    flat = pack_policy_weights(ac)
    grad = torch.zeros_like(flat)
    st = {k: {"exp_avg": torch.zeros_like(flat), "exp_avg_sq": torch.zeros_like(flat),
              "step": torch.zeros(1, dtype=torch.int32, device=dev)} for k in ("pi", "v")}
    norm = torch.zeros(1, dtype=torch.float64, device=dev)
    adam = lambda which, **kw: adam_step_device(
        flat, grad, st[which]["exp_avg"], st[which]["exp_avg_sq"], flat_slice(ac, which)[0],
        flat_slice(ac, which)[1] - flat_slice(ac, which)[0], st[which]["step"], pi_lr if which == "pi" else v_lr,
        B1, B2, EPS, max_grad_norm, **kw)
    pol = lambda **kw: policy_grad_device(flat, obs, act, lpo, adv, CLIP, summary, scratch, adv_moments=mom, **kw)
    loss_pi = pol(mu_out=mu_old).tolist()[1]
    loss_v = value_grad_device(flat, obs, ret, summary, scratch).tolist()[1]
    kl, clip_frac, stop = 0.0, 0.0, 0
    for i in range(iters):
        pol(grad=grad)
        adam("pi", norm_out=norm)
        s = pol(mu_old=mu_old).tolist()
        kl, clip_frac, stop = s[4], s[3], i + 1
        if kl > f32(target_kl):                              # the fp32 value the device compares with
            break
    for _ in range(v_iters):
        perm = torch.randperm(n, generator=generator, device=generator.device).to(dev)
        nb = min(num_mb, n)
        for k in range(nb):
            idx = perm[(k * n) // nb:((k + 1) * n) // nb].to(torch.int32)
            value_grad_device(flat, obs, ret, summary, scratch, grad=grad, idx=idx)
            adam("v")
    return flat, st, {"LossPi": loss_pi, "LossV": loss_v, "KL": kl, "ClipFrac": clip_frac, "StopIter": stop,
                      "GradNormPi": float(norm.item())}


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


CASES = {"a": (PI_LR_C, 1e9, "==12"), "b": (PI_LR_C, 0.0, "==1"), "c": (PI_LR_C, TARGET_KL_C, "inside")}


@pytest.mark.gpu
@pytest.mark.parametrize("case,d", [("a", 34), ("b", 34), ("c", 34), ("c", 42)])
def test_resident_update_is_the_literal_loop_bit_for_bit(gpu, lib, case, d):
    from cf2sim.ppo import ResidentPPOUpdater
    from cf2sim.rollout import pack_policy_weights
    pi_lr, target_kl, expect = CASES[case]
    ac_l, ro = gpu_rollout(11, gpu, d=d)
    assert ro.obs.shape[0] * ro.obs.shape[1] == 4120
    ac_r = copy.deepcopy(ac_l)
    gen = lambda: torch.Generator(device=gpu).manual_seed(17)
    flat_l, st, out_l = literal_update(ac_l, ro, pi_lr, 1e-3, target_kl, 12, 2, 16, gen(), max_grad_norm=MAX_NORM)
    print(case, d, out_l)
    if expect == "inside":
        assert 1 < out_l["StopIter"] < 12, out_l             # a condition on the inputs (module docstring)
    else:
        assert out_l["StopIter"] == int(expect[2:]), out_l
    up = ResidentPPOUpdater(ac_r, pi_lr, 1e-3, CLIP, target_kl, train_pi_iterations=12, train_v_iterations=2,
                            num_mini_batches=16, betas=(B1, B2), eps=EPS, max_grad_norm=MAX_NORM, generator=gen())
    out_r = up.update(ro)
    assert set(out_r) == {"LossPi", "LossV", "KL", "StopIter", "ClipFrac", "GradNormPi"}
    for k in out_l:
        assert out_r[k] == out_l[k], (k, out_r[k], out_l[k])
    assert bits_equal(up.flat, flat_l)
    assert bits_equal(pack_policy_weights(ac_r), flat_l)     # the module's tensors
    assert not bits_equal(pack_policy_weights(ac_l), flat_l)    # the literal loop left its module alone
    for which, opt in (("pi", up.pi_optimizer), ("v", up.v_optimizer)):
        assert bits_equal(opt.exp_avg, st[which]["exp_avg"]) and bits_equal(opt.exp_avg_sq, st[which]["exp_avg_sq"])
        assert torch.equal(opt.step_count, st[which]["step"])
    assert int(up.pi_optimizer.step_count.item()) == out_l["StopIter"] and int(up.v_optimizer.step_count.item()) == 32
    assert up.ctrl.tolist() == [0 if expect == "==12" else 1, out_l["StopIter"], 0, 0]


@pytest.mark.gpu
def test_second_update_and_resume(gpu, lib):
    from cf2sim.ppo import ResidentPPOUpdater
    from cf2sim.rollout import pack_policy_weights
    ac0, ro = gpu_rollout(11, gpu)
    _, ro2 = gpu_rollout(12, gpu)
    mk = lambda ac, gen: ResidentPPOUpdater(ac, PI_LR_C, 1e-3, CLIP, TARGET_KL_C, train_pi_iterations=12,
                                            train_v_iterations=2, max_grad_norm=MAX_NORM, generator=gen)
    ends = []
    for resume in (False, True):
        ac = copy.deepcopy(ac0)
        gen = torch.Generator(device=gpu).manual_seed(3)
        up = mk(ac, gen)
        first = up.update(ro)
        if resume:
            sd = up.state_dict()
            up = mk(ac, gen)
            assert int(up.pi_optimizer.step_count.item()) == 0
            up.load_state_dict(sd)
        second = up.update(ro2)
        assert int(up.pi_optimizer.step_count.item()) == first["StopIter"] + second["StopIter"]
        ends.append((pack_policy_weights(ac), up.pi_optimizer.exp_avg, up.pi_optimizer.exp_avg_sq, up.v_optimizer.exp_avg,
                     up.v_optimizer.exp_avg_sq, first, second))
    for a, b in zip(ends[0][:5], ends[1][:5]):
        assert bits_equal(a, b)
    assert ends[0][5:] == ends[1][5:]


@pytest.mark.gpu
def test_update_without_reading_never_synchronises(gpu, lib):
    from cf2sim.ppo import ResidentPPOUpdater
    ac, ro = gpu_rollout(11, gpu)
    up = ResidentPPOUpdater(ac, 3e-4, 1e-3, CLIP, 0.01, train_pi_iterations=4, train_v_iterations=1,
                            generator=torch.Generator(device=gpu).manual_seed(1))
    assert up.result() is None
    up.update(ro, read=False)                                # allocations and the library load happen here
    probe = torch.ones(1, device=gpu)
    mode = torch.cuda.get_sync_debug_mode()
    raised = None
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.item()
            raised = False
        except RuntimeError:
            raised = True
        if raised:
            assert up.update(ro, read=False) is None
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    out = up.result()
    assert out["StopIter"] >= 1 and math.isfinite(out["LossPi"]) and math.isfinite(out["GradNormPi"])
    if not raised:
        pytest.skip("this torch build does not raise on a synchronising call in sync debug mode 'error'")


@pytest.mark.gpu
def test_resident_updater_end_to_end_on_collected_data(gpu, lib):
    from cf2sim.ppo import ResidentPPOUpdater
    from cf2sim.rollout import FusedActorCritic, MLPActorCritic, collect
    from cf2sim.vec_env import BatchedCrazyflieEnv
    envs = BatchedCrazyflieEnv(ENV_ID, 256, seed=21, want_final_obs=True)
    torch.manual_seed(5)
    ac = MLPActorCritic().to(gpu)
    with torch.no_grad():
        ac.obs_oms.mean.normal_(0.0, 0.1)
        ac.obs_oms.std.uniform_(0.5, 1.5)
    fused = FusedActorCritic(ac, seed=2)
    ro = collect(envs, fused, 8)
    before = fused.w.clone()
    up = ResidentPPOUpdater(ac, 3e-4, 1e-3, CLIP, 0.01, train_pi_iterations=6, train_v_iterations=1, max_grad_norm=MAX_NORM,
                            fused=fused, generator=torch.Generator(device=gpu).manual_seed(17))
    out = up.update(ro)
    print(out)
    assert 1 <= out["StopIter"] <= 6 and out["GradNormPi"] > 0.0 and all(math.isfinite(v) for v in out.values())
    assert not torch.equal(fused.w, before)
    assert bits_equal(fused.w, FusedActorCritic(ac, seed=2).w)
    ro2 = collect(envs, fused, 8, obs=ro.last_obs, out=ro)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ro2.obs).all()) and bool(torch.isfinite(ro2.adv).all())
