"""TRPO and NPG updates: cf2_ppo_fisher_vec (csrc/cf2sim_ppo.hip), the solver kernels cf2_ng_cg_init,
cf2_ng_cg_step, cf2_ng_direction and cf2_ng_line_search (csrc/cf2sim_natgrad.hip) and, in cf2sim.ppo,
fisher_vec_torch, the torch restatements of the solver rules, the device wrappers and
NaturalGradientUpdater.

Tolerance rule (tests/test_ppo_update.py): per parameter tensor err = |x - x64|_inf / |x64|_inf against
the fp64 torch path on the CPU; the kernel may be at most max(8 x e32, 2^-20), e32 the same measure of
torch's fp32 path on the GPU on the same inputs.  Both are printed.  Dot products of the solver
kernels are held to |got - want| <= 2^-40 sum |a_i b_i| against an fp64 dot of the device's own vectors.

Without a GPU the torch path (NaturalGradientUpdater(device=False)) runs on synthetic_rollout(3)
(T = 6, N = 40, D = 34, stride 4, 10 CG iterations, damping 0.1) in fp64 and fp32.  Measured on the CPU
(fp64; fp32 agrees to 4 digits):

    target_kl   trial   KL        improvement   outcome
    0.01        0       0.00908   0.145         accepted
    1.0         0       2.235     --            rejected
    1.0         1       1.084     0.595         accepted
    3.0         0       18.45     --            rejected
    3.0         1       7.39      --            rejected
    3.0         2       3.204     0.295         accepted

Every decision has to be clear of its thresholds (a condition on the inputs): an accepted trial has
KL <= 0.9 x 1.5 target_kl and improvement >= 1e-3, a rejected one KL >= 1.1 x 1.5 target_kl or
improvement <= -1e-3.

Measured on an MI355X, worst parameter tensor, kernel / torch-fp32 (the full table is in DESIGN.md
section 8, "Natural-gradient updates on the device"):

    cf2_ppo_fisher_vec, random v    D = 34               D = 42
    m = 1                           2.7e-7 / 2.7e-7      2.6e-7 / 3.0e-7
    m = 15                          2.1e-7 / 1.6e-7      1.9e-7 / 1.9e-7
    m = 17                          1.9e-7 / 1.6e-7      1.6e-7 / 2.1e-7
    m = 1000                        1.1e-7 / 6.3e-7      1.1e-7 / 8.6e-7
    m = 70001                       6.6e-8 / 2.1e-6      7.0e-8 / 2.2e-6
    m = 250 of 1000, stride 4       1.3e-7 / 3.3e-7      1.3e-7 / 3.1e-7
    (v only in b3: 1.2e-7 .. 2.6e-7 / 1.3e-7 .. 2.5e-6; only in W1: 7.4e-8 .. 3.2e-7 / 1.8e-7 .. 2.7e-6)
    gradient with clip_ratio = inf  2.3e-7 .. 2.9e-7 / 2.6e-7 .. 8.7e-7
    10 CG steps: x                  0.8e-7 .. 1.2e-7 / 0.9e-7 .. 1.6e-7
                 r, p               2.8e-7 .. 7.5e-7 / 7.0e-7 .. 8.5e-7
    whole step, 240 rows            8.8e-5 / 4.1e-4
    whole step, 2 048 rows          5.6e-7 / 9.9e-6
"""
import copy
import ctypes
import dataclasses
import functools
import math
import os
import re

import pytest
import torch

from test_ppo_update import FLOOR, Dev, flat_to_tensors, module_grads, pool, rel_err, sizes, synthetic_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_ID = "DroneHoverBulletFreeEnvWithoutAdversary-v0"
NAMES = ("cf2_ppo_fisher_vec", "cf2_ng_cg_init", "cf2_ng_cg_step", "cf2_ng_direction", "cf2_ng_line_search")
INF = float("inf")
MS = (1, 15, 17, 1000, 70001)
SLICES = ((0, 4504), (3, 63))
WORDS = sizes(42)["v_end"] + 2 * 42
f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
DAMP, DECAY = f32(0.1), f32(0.8)
# (target_kl, line_search_steps, expected acceptance step) of the table above, then the all-rejected case
CASES = {"small": (0.01, 25, 1), "second": (1.0, 25, 2), "third": (3.0, 25, 3), "none": (1.0, 1, 0)}


@pytest.fixture(scope="module")
def lib():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    return _native.load()


def bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def cast_rollout(ro, dtype=None, device=None):
    from cf2sim.rollout import Rollout
    out = {}
    for f in dataclasses.fields(ro):
        if f.name == "storage":
            continue
        t = getattr(ro, f.name)
        if dtype is not None and t.is_floating_point():
            t = t.to(dtype)
        out[f.name] = t.to(device) if device is not None else t
    return Rollout(**out)


def pi_tensors(flat, d=34):
    return flat_to_tensors(flat, d, "pi")


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_natural_gradient_entry_points(lib):
    from cf2sim._native import EXPORTED_SYMBOLS
    txt = open(os.path.join(ROOT, "include", "cf2sim.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(cf2_\w+)\s*\(", txt, flags=re.M))
    out = os.popen(f"nm -D --defined-only {lib._name}").read()
    for name in NAMES:
        assert name in declared and name in EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported"
    assert lib.cf2_abi_version() == 8                       # additive change
    from cf2sim import ppo
    for k in ("RDOTR", "CG_STEPS", "CG_DONE", "XHX", "ALPHA", "EXPECTED", "STEP_FRAC", "ACCEPT_STEP", "LOSS_BEFORE",
              "LOSS_AFTER", "KL_AFTER", "PDOTZ", "BDOTB", "RESIDUAL"):
        assert int(re.search(rf"CF2_NG_{k} = (\d+)", txt).group(1)) == getattr(ppo, "NG_" + k), k
    assert int(re.search(r"CF2_NG_STATE_DOUBLES = (\d+)", txt).group(1)) == ppo.NG_STATE_DOUBLES


def test_host_error_paths_need_no_device(lib):
    host = (ctypes.c_double * 64)()                         # never dereferenced: every call returns first
    p = ctypes.addressof(host)
    p += -p % 16
    call = lambda fn, spec: (lambda **kw: fn(*[kw.get(k, v) for k, v in spec]))
    fvp = call(lib.cf2_ppo_fisher_vec, (
        ("w", p), ("d", 34), ("obs", p), ("n", 8), ("idx", None), ("m", 8), ("vec", p), ("out", p), ("summary", p),
        ("scratch", p), ("ctrl", None), ("stream", None)))
    for k in ("w", "obs", "vec", "out", "summary", "scratch"):
        assert fvp(**{k: None}) == -1, k
    for k in ("w", "idx", "vec", "out", "ctrl"):
        assert fvp(**{k: p + 2}) == -1, k
    for k in ("obs", "summary", "scratch"):
        assert fvp(**{k: p + 4}) == -1, k
    assert fvp(d=33) == -4 and fvp(d=35) == -4
    assert fvp(m=9) == -1 and fvp(n=0) == -1                # m > n without idx
    assert fvp(m=0) == 0 and fvp(m=0, w=None) == 0

    sl = (("begin", 0), ("count", 8))
    tail = (("state", p), ("ctrl", None), ("stream", None))
    init = call(lib.cf2_ng_cg_init, (("grad", p), ("b", p), ("x", p), ("r", p), ("p", p)) + sl + tail)
    step = call(lib.cf2_ng_cg_step, (("z", p), ("x", p), ("r", p), ("p", p)) + sl + (("damping", 0.1),) + tail)
    dirn = call(lib.cf2_ng_direction, (("z", p), ("x", p), ("b", p), ("step", p), ("w", p), ("old", p)) + sl +
                (("damping", 0.1), ("target_kl", 0.01)) + tail)
    ls = call(lib.cf2_ng_line_search, (("w", p), ("old", p), ("step", p)) + sl + (
        ("trial", 0), ("total", 25), ("decay", 0.8), ("target_kl", 0.01), ("eval", p), ("before", p), ("state", p),
        ("ctrl", p), ("stream", None)))
    for fn, ptrs, eight in ((init, ("grad", "b", "x", "r", "p"), ("state",)), (step, ("z", "x", "r", "p"), ("state",)),
                            (dirn, ("z", "x", "b", "step", "w", "old"), ("state",)),
                            (ls, ("w", "old", "step", "ctrl"), ("state", "eval", "before"))):
        for k in ptrs + eight:
            assert fn(**{k: None}) == -1, k
        for k in ptrs + (("ctrl",) if "ctrl" not in ptrs else ()):
            assert fn(**{k: p + 2}) == -1, k
        for k in eight:
            assert fn(**{k: p + 4}) == -1, k
        assert fn(begin=2 ** 32 - 4, count=8) == -1         # the slice runs past 32 bits
        assert fn(count=(1 << 20) + 1) == -4
        assert fn(count=0) == 0 and fn(count=0, state=None) == 0
    assert step(damping=-0.1) == -1 and step(damping=float("nan")) == -1
    assert dirn(damping=-0.1) == -1 and dirn(target_kl=-1.0) == -1 and dirn(target_kl=float("inf")) == -1
    assert ls(trial=25) == -1 and ls(decay=0.0) == -1 and ls(decay=1.5) == -1 and ls(target_kl=float("nan")) == -1


def test_fisher_identity_in_fp64():
    """Double-backward of the KL to the detached policy equals J^T Sigma^-1 J v / m."""
    from torch.func import functional_call, jvp, vjp
    from cf2sim.ppo import _standardized, fisher_vec_torch, pi_flat, pi_unflat
    ac, ro = synthetic_rollout(3)
    ac = ac.double()
    obs = ro.obs.reshape(-1, 34).double()[::4]
    m = obs.shape[0]
    v = torch.randn(sizes(34)["pi_end"], dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * 0.05
    got = fisher_vec_torch(ac, obs, v)
    names = [n for n, _ in ac.pi_net.named_parameters()]
    params = {n: q.detach() for n, q in ac.pi_net.named_parameters()}
    z = _standardized(ac, obs)
    f = lambda prm: functional_call(ac.pi_net, prm, (z,))
    tangents = dict(zip(names, [t.contiguous() for t in pi_unflat(ac, v)]))
    _, jv = jvp(f, (params,), (tangents,))
    _, pull = vjp(f, params)
    (jt,) = pull(jv * torch.exp(-2.0 * ac.log_std.detach()) / m)
    want = pi_flat(ac, [jt[n] for n in names])
    err = float((got - want).abs().max()) / float(want.abs().max())
    print(f"fisher identity: {err:.2e}")
    assert err <= 1e-12 and float(want.abs().max()) > 0


def run_torch_path(dtype, algorithm, target_kl, steps, v_iters=0):
    """NaturalGradientUpdater(device=False) on synthetic_rollout(3); returns the result, the module
    before and after, and every line-search trial as (trial, loss, kl, loss_before)."""
    import cf2sim.ppo as ppo
    ac, ro = synthetic_rollout(3)
    ac, ro = ac.to(dtype), cast_rollout(ro, dtype)
    before = copy.deepcopy(ac)
    trials, orig = [], ppo.line_search_torch
    try:
        ppo.line_search_torch = lambda j, total, decay, kl_t, loss, kl, lb: (
            trials.append((j, loss, kl, lb)), orig(j, total, decay, kl_t, loss, kl, lb))[1]
        up = ppo.NaturalGradientUpdater(ac, 1e-3, target_kl, algorithm=algorithm, line_search_steps=steps, device=False,
                                        train_v_iterations=v_iters, generator=torch.Generator().manual_seed(1))
        out = up.update(ro)
    finally:
        ppo.line_search_torch = orig
    return out, before, ac, trials


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", list(CASES))
def test_torch_path_trpo_accepts_where_the_table_says(case, dtype):
    from cf2sim.ppo import NaturalGradientUpdater
    target_kl, steps, want = CASES[case]
    out, before, ac, trials = run_torch_path(dtype, "trpo", target_kl, steps)
    print(case, dtype, out, trials)
    assert set(out) == set(NaturalGradientUpdater.KEYS) == {
        "LossPi", "LossV", "KL", "AcceptanceStep", "StepFrac", "xHx", "Alpha", "ExpectedImprove", "CGResidual", "GradNormPi"}
    assert out["AcceptanceStep"] == want
    assert len(trials) == (want if want else steps)
    for j, loss, kl, lb in trials:                           # the condition on the inputs
        if j + 1 == want:
            assert kl <= 0.9 * 1.5 * target_kl and lb - loss >= 1e-3, (j, loss, kl, lb)
        else:
            assert kl >= 1.1 * 1.5 * target_kl or lb - loss <= -1e-3, (j, loss, kl, lb)
    same = [same_bits(a.detach(), b.detach()) for a, b in zip(before.parameters(), ac.parameters())]
    if want == 0:
        assert all(same) and out["KL"] == 0.0 and out["StepFrac"] == 0.0
    else:
        assert abs(out["StepFrac"] - 0.8 ** (want - 1)) < 1e-12 and out["KL"] == trials[-1][2]
        assert not same_bits(before.pi_net[0].weight.detach(), ac.pi_net[0].weight.detach())
    assert out["xHx"] > 0 and out["ExpectedImprove"] > 0 and out["GradNormPi"] > out["CGResidual"] > 0
    assert abs(out["Alpha"] - math.sqrt(2 * target_kl / (out["xHx"] + 1e-8))) <= 1e-6 * out["Alpha"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_torch_path_npg_takes_the_full_step(dtype):
    from cf2sim.ppo import pi_flat
    out, before, ac, trials = run_torch_path(dtype, "npg", 0.01, 25, v_iters=1)
    print(dtype, out)
    assert trials == [] and out["AcceptanceStep"] == 1 and out["StepFrac"] == 1.0
    assert 0.005 <= out["KL"] <= 0.02                        # the quadratic model is only approximate
    moved = float((pi_flat(ac) - pi_flat(before)).double().norm())
    assert moved > 0 and not same_bits(before.v_net[0].weight.detach(), ac.v_net[0].weight.detach())
    trpo = run_torch_path(dtype, "trpo", 0.01, 25, v_iters=1)
    assert same_bits(pi_flat(trpo[2]), pi_flat(ac))          # TRPO's accepted trial 0 is NPG's step
    assert same_bits(trpo[2].v_net[0].weight.detach(), ac.v_net[0].weight.detach())


def test_solver_restatements_solve_a_small_system():
    from cf2sim.ppo import cg_init_torch, cg_step_torch, direction_torch
    g = torch.Generator().manual_seed(2)
    n = 12
    q = torch.randn(n, n, dtype=torch.float64, generator=g)
    A = q @ q.t() + n * torch.eye(n, dtype=torch.float64)
    grad = torch.randn(n, dtype=torch.float64, generator=g)
    st = cg_init_torch(grad)
    for _ in range(n):
        cg_step_torch(st, A @ st["p"], 0.25)
    # exact CG ends after n steps; the rule's 1e-6 terms in both quotients take over once r.r comes near
    # them, |r| ~ 1e-3, so the residual is held to ten times that, and r has to be the true residual
    res = -grad - (A @ st["x"] + 0.25 * st["x"])
    assert float(res.norm()) <= 1e-2 < 0.1 * float(grad.norm()) and float((res - st["r"]).norm()) <= 1e-9
    direction_torch(st, A @ st["x"], 0.25, 0.01)
    assert abs(float(0.5 * st["alpha"] ** 2 * st["xHx"]) - 0.01) < 1e-8      # the quadratic model's KL
    st = cg_init_torch(torch.full((5,), 1e4, dtype=torch.float64))
    cg_step_torch(st, st["p"].clone(), 0.0)                  # A = I converges at once
    frozen = {k: v.clone() for k, v in st.items() if isinstance(v, torch.Tensor)}
    cg_step_torch(st, st["p"].clone(), 0.0)
    assert st["done"] and st["steps"] == 1 and all(torch.equal(st[k], v) for k, v in frozen.items())


# ---------------------------------------------------------------------------------------------
# on the GPU: cf2_ppo_fisher_vec
# ---------------------------------------------------------------------------------------------
def direction_vec(d, kind):
    """A flat block: the policy slice holds the direction, every other word NaN."""
    S = sizes(d)
    g = torch.Generator().manual_seed(7 + d + len(kind))
    v = torch.zeros(S["pi_end"])
    if kind == "random":
        v = torch.randn(S["pi_end"], generator=g) * 0.05
    elif kind == "b3":
        b3 = S["pi"][2][3]
        v[b3:b3 + 4] = torch.randn(4, generator=g) * 0.05
    elif kind == "w1":
        v[:d * 50] = torch.randn(d * 50, generator=g) * 0.05
    full = torch.full((S["v_end"] + 2 * d,), float("nan"))
    full[:S["pi_end"]] = v
    return full


def fvp_reference(d, rows, kind, dtype, device):
    """(F v as parameter-shaped tensors, v.F v) of fisher_vec_torch in `dtype` on the pool's `rows`."""
    from cf2sim.ppo import fisher_vec_torch
    P, S = pool(d), sizes(d)
    ac = copy.deepcopy(P["ac"]).to(device=device, dtype=dtype)
    v = direction_vec(d, kind)[:S["pi_end"]].to(device=device, dtype=dtype)
    fv = fisher_vec_torch(ac, P["obs"][rows].to(device=device, dtype=dtype), v)
    return pi_tensors(fv, d), float(torch.dot(v, fv))


def check_fvp(lib, gpu, d, m, n, idx, label):
    from cf2sim.ppo import fisher_vec_device
    B = Dev(lib, gpu, d, m, n=n)
    S = sizes(d)
    rows = slice(0, m) if idx is None else idx.long()
    for kind in ("random", "b3", "w1"):
        vec_host = direction_vec(d, kind)
        vec, out = vec_host.to(gpu), torch.full_like(B.flat, float("nan"))
        summ = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        fisher_vec_device(B.flat, B.obs, vec, out, summ, B.scratch, idx=None if idx is None else idx.to(gpu), m=m)
        nan = torch.isnan(out)
        assert not bool(nan[:S["pi_end"]].any()) and bool(nan[S["pi_end"]:].all())
        assert same_bits(vec.cpu(), vec_host)
        g64, s64 = fvp_reference(d, rows, kind, torch.float64, "cpu")
        g32, s32 = fvp_reference(d, rows, kind, torch.float32, gpu)
        ek, e32 = rel_err(pi_tensors(out, d), g64), rel_err(g32, g64)
        print(f"{label} {kind} d={d} m={m}: kernel {max(ek):.3e} torch-fp32 {max(e32):.3e} per tensor "
              f"{['%.2e' % x for x in ek]} vs {['%.2e' % x for x in e32]}")
        for i, (a, b) in enumerate(zip(ek, e32)):
            assert a <= max(8.0 * b, FLOOR), (label, kind, d, m, i, a, b)
        ks = summ.tolist()
        assert ks[0] == float(m) and all(x == 0.0 for x in ks[2:]) and s64 > 0
        a, b = abs(ks[1] - s64) / s64, abs(s32 - s64) / s64
        print(f"   vFv kernel {a:.3e} torch-fp32 {b:.3e}")
        assert a <= max(8.0 * b, FLOOR), (label, kind, "vFv", d, m, ks[1], s64, s32)


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("d", [34, 42])
def test_fisher_vec_against_fp64(gpu, lib, d, m):
    check_fvp(lib, gpu, d, m, m, None, "fvp")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [34, 42])
def test_fisher_vec_on_every_fourth_row_against_fp64(gpu, lib, d):
    check_fvp(lib, gpu, d, 250, 1000, torch.arange(0, 1000, 4, dtype=torch.int32), "fvp stride 4")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [34, 42])
def test_fisher_vec_same_bits_twice_and_index_equals_dense(gpu, lib, d):
    from cf2sim.ppo import fisher_vec_device
    n, m = 5000, 1000
    B = Dev(lib, gpu, d, m, n=n)
    S = sizes(d)
    vec = direction_vec(d, "random").to(gpu)
    idx = torch.randint(0, n, (m,), generator=torch.Generator().manual_seed(8))
    idx[100:150] = idx[0:50]                                 # repeats
    idx[-1] = n - 1
    gathered = B.obs[idx.to(gpu)].contiguous()
    res = []
    for obs, kw in ((B.obs, {"idx": idx.to(gpu, dtype=torch.int32)}), (gathered, {}), (gathered, {})):
        out = torch.full_like(B.flat, float("nan"))
        summ = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        B.scratch.fill_(float(len(res)))                     # whatever the scratch held before
        fisher_vec_device(B.flat, obs, vec, out, summ, B.scratch, **kw)
        res.append((out, summ))
    for out, summ in res[1:]:
        assert same_bits(out, res[0][0]) and same_bits(summ, res[0][1])
    assert not bool(torch.isnan(res[0][0][:S["pi_end"]]).any()) and float(res[0][1][1]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("m", [17, 1000])
@pytest.mark.parametrize("d", [34, 42])
def test_unclipped_surrogate_gradient_against_fp64(gpu, lib, d, m):
    """clip_ratio = inf through policy_grad_device is -mean(ratio A): the surrogate TRPO uses."""
    from cf2sim.ppo import policy_grad_device, policy_terms_torch
    P = pool(d)
    B = Dev(lib, gpu, d, m)
    policy_grad_device(B.flat, B.obs, B.act, B.logp_old, B.adv, INF, B.summary, B.scratch, grad=B.grad, mu_old=B.mu_old)

    def ref(dtype, device):
        ac = copy.deepcopy(P["ac"]).to(device=device, dtype=dtype)
        c = lambda k: P[k][:m].to(device=device, dtype=dtype)
        for q in ac.parameters():
            q.grad = None
        ratio = policy_terms_torch(ac, c("obs"), c("act"), c("logp_old"), c("adv"), 0.2)["ratio"]
        loss = -(ratio * c("adv")).mean()
        loss.backward()
        return module_grads(ac, "pi"), float(loss.detach())

    g64, l64 = ref(torch.float64, "cpu")
    g32, l32 = ref(torch.float32, gpu)
    ek, e32 = rel_err(pi_tensors(B.grad, d), g64), rel_err(g32, g64)
    print(f"clip=inf d={d} m={m}: kernel {max(ek):.3e} torch-fp32 {max(e32):.3e}")
    for i, (a, b) in enumerate(zip(ek, e32)):
        assert a <= max(8.0 * b, FLOOR), (d, m, i, a, b)
    ks = B.summary.tolist()
    a, b = abs(ks[1] - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    print(f"   loss kernel {a:.3e} torch-fp32 {b:.3e}")
    assert ks[0] == float(m) and ks[3] == 0.0 and a <= max(8.0 * b, FLOOR), (ks, l64, l32)


# ---------------------------------------------------------------------------------------------
# on the GPU: the solver kernels
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spd_case(begin, count):
    """A fixed SPD operator A = diag + U U^T on the slice, a gradient, and the CG recurrence of
    cf2sim.ppo's restatements in fp64 (the reference) and fp32 (the yardstick), 10 steps."""
    from cf2sim.ppo import cg_init_torch, cg_step_torch, direction_torch
    g = torch.Generator().manual_seed(500 + begin + count)
    diag = torch.rand(count, dtype=torch.float64, generator=g) * 1.5 + 0.5
    U = torch.randn(count, 6, dtype=torch.float64, generator=g) / math.sqrt(count)
    grad = torch.randn(WORDS, generator=g) * 0.05
    theta = torch.randn(WORDS, generator=g) * 0.3
    sl = slice(begin, begin + count)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        A = lambda v: (diag.to(dtype) * v + U.to(dtype) @ (U.to(dtype).t() @ v))
        st = cg_init_torch(grad[sl].to(dtype))
        for _ in range(10):
            cg_step_torch(st, A(st["p"]), DAMP)
        direction_torch(st, A(st["x"]), DAMP, f32(0.01))
        ref[dtype] = st
    apply64 = lambda v: diag * v + U @ (U.t() @ v)
    return {"apply": apply64, "grad": grad, "theta": theta, "ref": ref}


def canaried(values, begin, count, gpu):
    t = torch.full((WORDS,), float("nan"))
    t[begin:begin + count] = values
    return t.to(gpu)


def outside_is_nan(t, begin, count):
    mask = torch.ones(WORDS, dtype=torch.bool)
    mask[begin:begin + count] = False
    c = t.cpu()
    return bool(torch.isnan(c[mask]).all()) and not bool(torch.isnan(c[begin:begin + count]).any())


def dot_ok(got, a, b):
    want = float(torch.dot(a, b))
    return abs(got - want) <= 2.0 ** -40 * float((a * b).abs().sum()), (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("begin,count", SLICES)
def test_cg_and_direction_against_fp64(gpu, lib, begin, count):
    from cf2sim import ppo
    C = spd_case(begin, count)
    sl = slice(begin, begin + count)
    nanb = lambda: torch.full((WORDS,), float("nan"), device=gpu)
    grad = canaried(C["grad"][sl], begin, count, gpu)
    b, x, r, p, z, step, old = (nanb() for _ in range(7))
    st = torch.full((16,), float("nan"), dtype=torch.float64, device=gpu)
    ppo.ng_cg_init_device(grad, b, x, r, p, begin, count, st)
    s = st.tolist()
    b64 = -C["grad"][sl].double()
    ok, info = dot_ok(s[ppo.NG_RDOTR], b64, b64)
    assert ok, info
    assert s[ppo.NG_BDOTB] == s[ppo.NG_RDOTR] == s[ppo.NG_RESIDUAL]
    assert all(v == 0.0 for i, v in enumerate(s) if i not in (ppo.NG_RDOTR, ppo.NG_BDOTB, ppo.NG_RESIDUAL))
    assert same_bits(b[sl].cpu(), -C["grad"][sl]) and same_bits(r[sl], b[sl]) and same_bits(p[sl], b[sl])
    assert not bool(x[sl].any())
    for k in range(10):
        p64 = p[sl].double().cpu()
        zk = C["apply"](p64).float()                         # z = A p from the host, as an fp32 block
        z[sl] = zk.to(gpu)
        rd_before = st[ppo.NG_RDOTR].item()
        ppo.ng_cg_step_device(z, x, r, p, begin, count, DAMP, st)
        s = st.tolist()
        ok, info = dot_ok(s[ppo.NG_PDOTZ], p64, zk.double() + DAMP * p64)
        assert ok, (k, info)
        r64 = r[sl].double().cpu()
        ok, info = dot_ok(s[ppo.NG_RESIDUAL], r64, r64)
        assert ok, (k, info)
        assert s[ppo.NG_CG_STEPS] == k + 1 and s[ppo.NG_CG_DONE] == 0.0 and s[ppo.NG_RDOTR] == s[ppo.NG_RESIDUAL]
        assert rd_before > 0
    want, yard = C["ref"][torch.float64], C["ref"][torch.float32]
    for name, got in (("x", x), ("r", r), ("p", p)):
        ek, e32 = rel_err([got[sl]], [want[name]])[0], rel_err([yard[name]], [want[name]])[0]
        print(f"cg [{begin}, {begin + count}) {name}: kernel {ek:.3e} torch-fp32 {e32:.3e}")
        assert ek <= max(8.0 * e32, FLOOR), (name, ek, e32)
    # the direction
    x64 = x[sl].double().cpu()
    zx = C["apply"](x64).float()
    z[sl] = zx.to(gpu)
    theta = canaried(C["theta"][sl], begin, count, gpu)
    kl_t = f32(0.01)
    ppo.ng_direction_device(z, x, b, step, theta, old, begin, count, DAMP, kl_t, st)
    s = st.tolist()
    ok, info = dot_ok(s[ppo.NG_XHX], x64, zx.double() + DAMP * x64)
    assert ok, info
    alpha = math.sqrt(2.0 * kl_t / (s[ppo.NG_XHX] + 1e-8))
    assert abs(s[ppo.NG_ALPHA] - alpha) <= 2.0 ** -40 * alpha
    step64 = step[sl].double().cpu()
    ok, info = dot_ok(s[ppo.NG_EXPECTED], b64, step64)
    assert ok, info
    assert same_bits(step[sl].cpu(), (s[ppo.NG_ALPHA] * x64).float())
    assert same_bits(old[sl].cpu(), C["theta"][sl])
    assert same_bits(theta[sl].cpu(), (C["theta"][sl].double() + step64).float())
    ek, e32 = rel_err([step[sl]], [want["step"]])[0], rel_err([yard["step"]], [want["step"]])[0]
    print(f"direction [{begin}, {begin + count}) step: kernel {ek:.3e} torch-fp32 {e32:.3e}")
    assert ek <= max(8.0 * e32, FLOOR), (ek, e32)
    for name, key in (("xHx", ppo.NG_XHX), ("alpha", ppo.NG_ALPHA), ("expected", ppo.NG_EXPECTED)):
        w = float(want[name])
        ek, e32 = abs(s[key] - w) / abs(w), abs(float(yard[name]) - w) / abs(w)
        print(f"   {name}: kernel {ek:.3e} torch-fp32 {e32:.3e}")
        assert ek <= max(8.0 * e32, FLOOR), (name, ek, e32)
    for t in (grad, b, x, r, p, z, step, theta, old):        # the canaries
        assert outside_is_nan(t, begin, count)


@pytest.mark.gpu
@pytest.mark.parametrize("begin,count", SLICES)
def test_cg_with_the_identity_converges_in_one_step_and_then_writes_nothing(gpu, lib, begin, count):
    from cf2sim import ppo
    sl = slice(begin, begin + count)
    grad = canaried(torch.randn(count, generator=torch.Generator().manual_seed(count)) * 1e4, begin, count, gpu)
    b, x, r, p = (torch.full((WORDS,), float("nan"), device=gpu) for _ in range(4))
    st = torch.zeros(16, dtype=torch.float64, device=gpu)
    ppo.ng_cg_init_device(grad, b, x, r, p, begin, count, st)
    ppo.ng_cg_step_device(p.clone(), x, r, p, begin, count, 0.0, st)       # z = I p
    s = st.tolist()
    assert s[ppo.NG_CG_DONE] == 1.0 and s[ppo.NG_CG_STEPS] == 1.0 and math.sqrt(s[ppo.NG_RESIDUAL]) < 1e-10
    assert s[ppo.NG_RDOTR] == s[ppo.NG_BDOTB] > 0            # rdotr and p stay
    assert same_bits(p[sl], b[sl])
    assert float((x[sl] - b[sl]).abs().max()) <= 2.0 ** -23 * float(b[sl].abs().max())
    keep = [t.clone() for t in (x, r, p, st)]
    ppo.ng_cg_step_device(torch.ones_like(p), x, r, p, begin, count, 0.0, st)
    for a, k in zip((x, r, p, st), keep):
        assert same_bits(a, k)
    for t in (b, x, r, p):
        assert outside_is_nan(t, begin, count)


@pytest.mark.gpu
@pytest.mark.parametrize("begin,count", SLICES)
def test_line_search_branches(gpu, lib, begin, count):
    from cf2sim import ppo
    g = torch.Generator().manual_seed(40 + count)
    sl = slice(begin, begin + count)
    old_h, step_h, trial_h = (torch.randn(count, generator=g) * s for s in (0.3, 0.01, 0.3))
    kl_t = f32(0.01)
    d64 = float(DECAY)

    def run(trial, total, loss, kl, before=1.0, ctrl0=0):
        theta, old, step = (canaried(v, begin, count, gpu) for v in (trial_h, old_h, step_h))
        st = torch.full((16,), -5.0, dtype=torch.float64, device=gpu)
        ctrl = torch.tensor([ctrl0, 0, 0, 0], dtype=torch.int32, device=gpu)
        summ = torch.tensor([240.0, loss, 0.0, 0.0, kl, 1.0, 0.0, 0.0], dtype=torch.float64, device=gpu)
        lb = torch.tensor([before], dtype=torch.float64, device=gpu)
        ppo.ng_line_search_device(theta, old, step, begin, count, trial, total, DECAY, kl_t, summ, lb, st, ctrl)
        for t in (theta, old, step):
            assert outside_is_nan(t, begin, count)
        assert same_bits(old[sl].cpu(), old_h) and same_bits(step[sl].cpu(), step_h)
        return theta[sl].cpu(), st.tolist(), ctrl.tolist()

    power = lambda e: 1.0 if e == 0 else d64 if e == 1 else d64 * d64            # e <= 2: as repeated squaring
    retry = lambda e: (old_h.double() + power(e) * step_h.double()).float()
    untouched = [-5.0] * 16
    for what, loss, kl in (("nan loss", float("nan"), 0.001), ("inf loss", INF, 0.001), ("worse loss", 1.0 + 1e-9, 0.001),
                           ("kl too large", 0.5, math.nextafter(1.5 * kl_t, INF)), ("nan kl", 0.5, float("nan"))):
        for trial in (0, 1):
            theta, st, ctrl = run(trial, 25, loss, kl)
            assert same_bits(theta, retry(trial + 1)) and st == untouched and ctrl == [0, 0, 0, 0], (what, trial)
    for trial, loss, kl in ((0, 1.0, 1.5 * kl_t), (2, 0.25, 0.0)):       # accept: both comparisons are inclusive
        theta, st, ctrl = run(trial, 25, loss, kl)
        assert same_bits(theta, trial_h) and ctrl == [1, trial + 1, 0, 0]
        want = list(untouched)
        want[ppo.NG_STEP_FRAC], want[ppo.NG_ACCEPT_STEP] = power(trial), float(trial + 1)
        want[ppo.NG_LOSS_BEFORE], want[ppo.NG_LOSS_AFTER], want[ppo.NG_KL_AFTER] = 1.0, loss, kl
        assert st == want, (trial, st)
    for trial, total in ((0, 1), (24, 25)):                  # the last trial rejected: theta_old comes back
        theta, st, ctrl = run(trial, total, 2.0, 0.001, before=0.75)
        assert same_bits(theta, old_h) and ctrl == [1, 0, 0, 0]
        want = list(untouched)
        want[ppo.NG_STEP_FRAC], want[ppo.NG_ACCEPT_STEP], want[ppo.NG_KL_AFTER] = 0.0, 0.0, 0.0
        want[ppo.NG_LOSS_BEFORE], want[ppo.NG_LOSS_AFTER] = 0.75, 0.75
        assert st == want, (trial, st)
    theta, st, ctrl = run(3, 25, 0.25, 0.0, ctrl0=1)         # stopped: nothing written
    assert same_bits(theta, trial_h) and st == untouched and ctrl == [1, 0, 0, 0]


@pytest.mark.gpu
def test_gate_leaves_everything_untouched(gpu, lib):
    from cf2sim import ppo
    d, m, begin, count = 34, 1000, 3, 63
    B = Dev(lib, gpu, d, m)
    ctrl = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=gpu)
    vec = direction_vec(d, "random").to(gpu)
    out = torch.full_like(B.flat, float("nan"))
    summ = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
    B.scratch.fill_(-3.0)
    ppo.fisher_vec_device(B.flat, B.obs, vec, out, summ, B.scratch, ctrl=ctrl)
    assert bool(torch.isnan(out).all()) and bool((summ == 7.0).all()) and bool((B.scratch == -3.0).all())
    opened = torch.zeros(4, dtype=torch.int32, device=gpu)
    out2, out3 = torch.full_like(out, float("nan")), torch.full_like(out, float("nan"))
    ppo.fisher_vec_device(B.flat, B.obs, vec, out2, summ, B.scratch, ctrl=opened)
    ppo.fisher_vec_device(B.flat, B.obs, vec, out3, summ.clone(), B.scratch)
    assert same_bits(out2, out3) and float(summ[0]) == m     # an open gate is the ungated call
    blocks = [torch.full((WORDS,), float(k + 1), device=gpu) for k in range(7)]
    st = torch.full((16,), -5.0, dtype=torch.float64, device=gpu)
    keep = [t.clone() for t in blocks + [st]]
    g, b, x, r, p, z, step = blocks
    ppo.ng_cg_init_device(g, b, x, r, p, begin, count, st, ctrl=ctrl)
    ppo.ng_cg_step_device(z, x, r, p, begin, count, DAMP, st, ctrl=ctrl)
    ppo.ng_direction_device(z, x, b, step, g, r, begin, count, DAMP, 0.01, st, ctrl=ctrl)
    ppo.ng_line_search_device(g, r, step, begin, count, 0, 25, DECAY, 0.01, summ, summ[1:2], st, ctrl)
    for a, k in zip(blocks + [st], keep):
        assert same_bits(a, k)
    assert ctrl.tolist() == [1, 0, 0, 0]
    with pytest.raises(ValueError):
        ppo.ng_cg_step_device(z, x, r, p, WORDS - 10, 11, DAMP, st)
    with pytest.raises(ValueError):
        ppo.ng_line_search_device(g, r, step, begin, count, 0, 25, DECAY, 0.01, summ, summ[1:2], st, None)


# ---------------------------------------------------------------------------------------------
# on the GPU: NaturalGradientUpdater
# ---------------------------------------------------------------------------------------------
def gpu_rollout(seed, gpu, T=6, N=40, d=34):
    ac, ro = synthetic_rollout(seed, T=T, N=N, d=d)
    return ac.to(gpu), cast_rollout(ro, device=gpu)


def literal_update(ac, ro, target_kl, algorithm, ls_steps, v_iters, generator, v_lr=1e-3):
    """The update from the same kernels driven by the host: a read after every step, nothing launched
    past an accept.  Returns the flat block, ng_state and the log entries."""
    from cf2sim import _native, ppo
    from cf2sim.rollout import pack_policy_weights
    lib = _native.load()
    d = ro.obs.shape[-1]
    obs, act = ro.obs.reshape(-1, d).contiguous(), ro.act.reshape(-1, 4).contiguous()
    lpo, adv, ret = (t.reshape(-1).contiguous() for t in (ro.logp, ro.adv, ro.ret))
    n, dev = obs.shape[0], obs.device
    nbytes = max(lib.cf2_ppo_scratch_bytes(n, d), lib.cf2_column_moments_scratch_bytes(n, 1))
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    mom = torch.empty(2, dtype=torch.float64, device=dev)
    summary, summary0, summary_f = (torch.zeros(8, dtype=torch.float64, device=dev) for _ in range(3))
    mu_old = torch.empty(n, 4, device=dev)
    assert lib.cf2_column_moments(adv.data_ptr(), n, 1, mom.data_ptr(), scratch.data_ptr(), None) == 0
    flat = pack_policy_weights(ac)
    grad = torch.zeros_like(flat)
    b, x, r, p, z, step, old = (torch.zeros_like(flat) for _ in range(7))
    st = torch.zeros(16, dtype=torch.float64, device=dev)
    ctrl = torch.zeros(4, dtype=torch.int32, device=dev)
    p0, p1 = ppo.flat_slice(ac, "pi")
    v0, v1 = ppo.flat_slice(ac, "v")
    fidx = torch.arange(0, n, 4, dtype=torch.int32, device=dev)
    pol = lambda summ, **kw: ppo.policy_grad_device(flat, obs, act, lpo, adv, INF, summ, scratch, adv_moments=mom, **kw)
    loss_v = ppo.value_grad_device(flat, obs, ret, summary, scratch).tolist()[1]
    loss_pi = pol(summary0, mu_out=mu_old, grad=grad).tolist()[1]
    ppo.ng_cg_init_device(grad, b, x, r, p, p0, p1 - p0, st)
    for _ in range(10):
        ppo.fisher_vec_device(flat, obs, p, z, summary_f, scratch, idx=fidx)
        ppo.ng_cg_step_device(z, x, r, p, p0, p1 - p0, 0.1, st)
        assert st[ppo.NG_CG_DONE].item() == 0.0
    ppo.fisher_vec_device(flat, obs, x, z, summary_f, scratch, idx=fidx)
    ppo.ng_direction_device(z, x, b, step, flat, old, p0, p1 - p0, 0.1, target_kl, st)
    if algorithm == "trpo":
        for j in range(ls_steps):
            pol(summary, mu_old=mu_old)
            ppo.ng_line_search_device(flat, old, step, p0, p1 - p0, j, ls_steps, 0.8, target_kl, summary, summary0[1:2],
                                      st, ctrl)
            if ctrl.tolist()[0]:
                break
        s = st.tolist()
        kl, acc, frac = s[ppo.NG_KL_AFTER], int(s[ppo.NG_ACCEPT_STEP]), s[ppo.NG_STEP_FRAC]
    else:
        kl, acc, frac = pol(summary, mu_old=mu_old).tolist()[4], 1, 1.0
    adam = {k: torch.zeros_like(flat) for k in ("m", "v")}
    vstep = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(v_iters):
        perm = torch.randperm(n, generator=generator, device=generator.device).to(dev)
        nb = min(16, n)
        for k in range(nb):
            idx = perm[(k * n) // nb:((k + 1) * n) // nb].to(torch.int32)
            ppo.value_grad_device(flat, obs, ret, summary_f, scratch, grad=grad, idx=idx)
            ppo.adam_step_device(flat, grad, adam["m"], adam["v"], v0, v1 - v0, vstep, v_lr)
    s = st.tolist()
    return flat, st, {"LossPi": loss_pi, "LossV": loss_v, "KL": kl, "AcceptanceStep": acc, "StepFrac": frac,
                      "xHx": s[ppo.NG_XHX], "Alpha": s[ppo.NG_ALPHA], "ExpectedImprove": s[ppo.NG_EXPECTED],
                      "CGResidual": math.sqrt(s[ppo.NG_RESIDUAL]), "GradNormPi": math.sqrt(s[ppo.NG_BDOTB])}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES) + ["npg"])
def test_resident_sequence_is_the_literal_loop_bit_for_bit(gpu, lib, case):
    from cf2sim.ppo import NaturalGradientUpdater
    from cf2sim.rollout import pack_policy_weights
    target_kl, steps, want = CASES[case] if case != "npg" else (0.01, 25, 1)
    algorithm = "npg" if case == "npg" else "trpo"
    ac_l, ro = gpu_rollout(3, gpu)
    assert ro.obs.shape[0] * ro.obs.shape[1] == 240          # the products run on 60 rows: 3 tiles and 12 rows
    ac_r = copy.deepcopy(ac_l)
    gen = lambda: torch.Generator(device=gpu).manual_seed(17)
    flat_l, st_l, out_l = literal_update(ac_l, ro, target_kl, algorithm, steps, 1, gen())
    print(case, out_l)
    assert out_l["AcceptanceStep"] == want
    up = NaturalGradientUpdater(ac_r, 1e-3, target_kl, algorithm=algorithm, line_search_steps=steps, train_v_iterations=1,
                                generator=gen())
    out_r = up.update(ro)
    assert set(out_r) == set(out_l)
    for k in out_l:
        assert out_r[k] == out_l[k], (k, out_r[k], out_l[k])
    assert same_bits(up.flat, flat_l) and same_bits(up.ng_state, st_l)
    assert same_bits(pack_policy_weights(ac_r), flat_l)      # the module's tensors
    moved = not same_bits(pack_policy_weights(ac_l)[:sizes(34)["pi_end"]], flat_l[:sizes(34)["pi_end"]])
    assert moved == (want != 0)                              # all rejected: the policy is back bit for bit
    if algorithm == "trpo":
        assert up.ctrl.tolist() == [1, want, 0, 0]
    assert int(up.v_optimizer.step_count.item()) == 16 and set(up.state_dict()) == {"v"}


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(6, 40), (8, 256)])
def test_device_path_follows_the_torch_path(gpu, lib, T, N):
    from cf2sim.ppo import NaturalGradientUpdater, pi_flat
    res = {}
    for name, dtype, dev, device in (("ref", torch.float64, "cpu", False), ("t32", torch.float32, gpu, False),
                                     ("dev", torch.float32, gpu, True)):
        ac, ro = synthetic_rollout(3, T=T, N=N)
        ac, ro = ac.to(device=dev, dtype=dtype), cast_rollout(ro, dtype, dev)
        old = pi_flat(ac).clone()
        up = NaturalGradientUpdater(ac, 1e-3, 0.01, algorithm="trpo", train_v_iterations=0, device=device)
        out = up.update(ro)
        res[name] = (pi_tensors(pi_flat(ac).double().cpu() - old.double().cpu()), out)
    want, ref = res["ref"]
    ek, e32 = rel_err(res["dev"][0], want), rel_err(res["t32"][0], want)
    print(f"step, {T * N} rows: kernel {max(ek):.3e} torch-fp32 {max(e32):.3e} per tensor "
          f"{['%.2e' % x for x in ek]} vs {['%.2e' % x for x in e32]}")
    print(ref, res["dev"][1])
    for i, (a, b) in enumerate(zip(ek, e32)):
        assert a <= max(8.0 * b, FLOOR), (i, a, b)
    out = res["dev"][1]
    assert out["AcceptanceStep"] == ref["AcceptanceStep"] == res["t32"][1]["AcceptanceStep"] == 1
    for k in ("LossPi", "KL"):
        assert abs(out[k] - ref[k]) <= 1e-4 * max(abs(ref[k]), 1e-3), (k, out[k], ref[k])


@pytest.mark.gpu
def test_update_without_reading_never_synchronises(gpu, lib):
    from cf2sim.ppo import NaturalGradientUpdater
    ac, ro = gpu_rollout(3, gpu)
    up = NaturalGradientUpdater(ac, 1e-3, 1.0, line_search_steps=4, train_v_iterations=1,
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
    assert out["AcceptanceStep"] >= 0 and math.isfinite(out["LossPi"]) and math.isfinite(out["GradNormPi"])
    if not raised:
        pytest.skip("this torch build does not raise on a synchronising call in sync debug mode 'error'")


@pytest.mark.gpu
def test_natural_gradient_end_to_end_on_collected_data(gpu, lib):
    from cf2sim.ppo import NaturalGradientUpdater
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
    for algorithm in ("trpo", "npg"):
        before = fused.w.clone()
        up = NaturalGradientUpdater(ac, 1e-3, 0.01, algorithm=algorithm, train_v_iterations=1, fused=fused,
                                    generator=torch.Generator(device=gpu).manual_seed(17))
        out = up.update(ro)
        print(algorithm, out)
        assert all(math.isfinite(v) for v in out.values()) and out["GradNormPi"] > 0 and out["xHx"] > 0
        assert 0 <= out["AcceptanceStep"] <= 25 and (out["KL"] <= 1.5 * 0.01 if algorithm == "trpo" else out["KL"] > 0)
        assert not torch.equal(fused.w, before)
        assert same_bits(fused.w, FusedActorCritic(ac, seed=2).w)
    ro2 = collect(envs, fused, 8, obs=ro.last_obs, out=ro)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ro2.obs).all()) and bool(torch.isfinite(ro2.adv).all())
