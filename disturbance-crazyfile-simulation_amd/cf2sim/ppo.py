"""The PPO update on a batched rollout: the reference's ``update`` --
``train_pi_iterations`` full-batch policy iterations with a KL check after each, then
``train_v_iterations`` passes of ``num_mini_batches`` value mini-batches -- with loss and gradient of
both networks from the fused HIP kernels of csrc/cf2sim_ppo.hip (cf2_ppo_policy_grad,
cf2_ppo_value_grad) and a torch optimiser on the module's parameters (``PPOUpdater``), or with the
optimiser and the KL stop on the device too (``ResidentPPOUpdater``: cf2_adam_step of
csrc/cf2sim_optim.hip on the flat weight block, cf2_ppo_policy_grad_gated).

Reference behaviour restated (paths relative to phoenix_drone_simulation/algs/):

* ``compute_loss_pi`` (ppo/ppo.py): ratio = exp(logp - logp_old), loss = -mean(min(ratio A,
  clamp(ratio, 1 - c, 1 + c) A)) minus an entropy term.  The entropy of the Gaussian depends on
  log_std only, which is not trained (requires_grad=False, annealed by ``set_log_std``), so the term
  has no gradient and is left out.
* The buffer's ``get()`` standardises the advantages, (adv - mean) / (std + 1e-8) (core.py); here the
  moments come from cf2_column_moments and the kernel standardises on the fly.
* ``update_policy_net`` (iwpg/iwpg.py): after every optimiser step the KL divergence between the
  policy before the update and the current one is read on the host; the loop stops once it exceeds
  ``target_kl``.  For two Gaussians with the same (untrained) sigma the KL is exactly
  sum_k (mu_old_k - mu_k)^2 / (2 sigma_k^2).
* ``update_value_net``: mean squared error against the value targets over shuffled mini-batches.

``policy_loss_torch`` / ``value_loss_torch`` restate the two losses in differentiable torch: they
are the path of ``PPOUpdater(device=False)`` (any device, also the CPU) and the reference the
kernels are tested against.
"""
from __future__ import annotations

import torch
from torch import nn

from .rollout import MLPActorCritic, Rollout, pack_policy_weights

_LOG_SQRT_2PI = 0.91893853320467274


def _standardized(ac: MLPActorCritic, obs: torch.Tensor) -> torch.Tensor:
    """(obs - mean) * scale with the flat block's scale, 1 / (std + eps) in fp64 rounded to fp32, as
    ``pack_policy_weights`` stores it and the kernels apply it."""
    if ac.obs_oms is None:
        return obs
    scale = (1.0 / (ac.obs_oms.std.detach().double() + ac.obs_oms.eps)).float()
    return (obs - ac.obs_oms.mean.detach().to(obs.dtype)) * scale.to(obs.dtype)


def policy_terms_torch(ac: MLPActorCritic, obs, act, logp_old, adv, clip_ratio: float, mu_old=None) -> dict:
    """Per-row terms of the clipped surrogate: mu, logp, ratio, the row losses and (with mu_old) the
    exact Gaussian KL.  Differentiable in ac.pi_net's parameters; any dtype and device."""
    mu = ac.pi_net(_standardized(ac, obs))
    log_std = ac.log_std.detach().to(mu.dtype)
    z = (act - mu) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std - _LOG_SQRT_2PI).sum(-1)
    ratio = torch.exp(logp - logp_old)
    rows = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip_ratio, 1.0 + clip_ratio) * adv)
    out = {"mu": mu, "logp": logp, "ratio": ratio, "rows": rows}
    if mu_old is not None:
        out["kl"] = ((mu_old - mu) ** 2 * (0.5 * torch.exp(-2.0 * log_std))).sum(-1)
    return out


def policy_loss_torch(ac: MLPActorCritic, obs, act, logp_old, adv, clip_ratio: float) -> torch.Tensor:
    """-mean(min(ratio A, clamp(ratio, 1 - c, 1 + c) A)): compute_loss_pi without the entropy term."""
    return policy_terms_torch(ac, obs, act, logp_old, adv, clip_ratio)["rows"].mean()


def value_loss_torch(ac: MLPActorCritic, obs, target) -> torch.Tensor:
    """mean((V(obs) - target)^2)."""
    return ((ac.v_net(_standardized(ac, obs)).squeeze(-1) - target) ** 2).mean()


def _linears(ac: MLPActorCritic, which: str):
    if which not in ("pi", "v"):
        raise ValueError(f"which must be 'pi' or 'v', got {which!r}")
    net = ac.pi_net if which == "pi" else ac.v_net
    return [m for m in net if isinstance(m, nn.Linear)]


def flat_slice(ac: MLPActorCritic, which: str) -> tuple[int, int]:
    """[begin, end) of the pi or v parameters in the flat block of ``pack_policy_weights``
    (pi: W1 b1 W2 b2 W3 b3; the four log_std words; then v likewise)."""
    n_pi = sum(m.weight.numel() + m.bias.numel() for m in _linears(ac, "pi"))
    if which == "pi":
        return 0, n_pi
    begin = n_pi + ac.log_std.numel()
    return begin, begin + sum(m.weight.numel() + m.bias.numel() for m in _linears(ac, "v"))


@torch.no_grad()
def scatter_flat_grad(ac: MLPActorCritic, flat: torch.Tensor, which: str) -> None:
    """Write the pi or v slice of a flat gradient (the layout of ``pack_policy_weights``: matrices
    input-major, i.e. transposed) into ``.grad`` of ac.pi_net's / ac.v_net's parameters."""
    off, end = flat_slice(ac, which)
    for m in _linears(ac, which):
        for p, src in ((m.weight, flat[off:off + m.weight.numel()].view(m.in_features, m.out_features).t()),
                       (m.bias, flat[off + m.weight.numel():off + m.weight.numel() + m.bias.numel()])):
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.copy_(src)
        off += m.weight.numel() + m.bias.numel()
    assert off == end


def _check_common(lib, flat, obs, n, idx, m, grad, summary, scratch):
    from .vec_env import _check_buf
    dev, f32 = flat.device, torch.float32
    if dev.type != "cuda":
        raise ValueError("the PPO gradient kernels need buffers on the GPU")
    d = obs.shape[-1] if obs.dim() == 2 else -1
    if d not in (34, 42):
        raise ValueError(f"obs must be [n, 34] or [n, 42], got {tuple(obs.shape)}")
    count = lib.cf2_policy_weights_count(d)
    _check_buf(flat, "flat", (count,), f32, dev)
    _check_buf(obs, "obs", (n, d), f32, dev, align=8)
    if idx is not None:
        _check_buf(idx, "idx", (m,), torch.int32, dev)
    elif m > n:
        raise ValueError(f"m = {m} rows of n = {n} need idx")
    _check_buf(grad, "grad", (count,), f32, dev)
    if summary is None:
        raise ValueError("summary is required")
    _check_buf(summary, "summary", (8,), torch.float64, dev, align=8)
    need = lib.cf2_ppo_scratch_bytes(m, d)
    if scratch is None or not isinstance(scratch, torch.Tensor) or scratch.device != dev or not scratch.is_contiguous() \
            or scratch.data_ptr() % 8 or scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"scratch must be a contiguous 8-byte aligned tensor of at least {need} bytes on {dev}")
    return d, dev


def policy_grad_device(flat, obs, act, logp_old, adv, clip_ratio: float, summary, scratch, grad=None, idx=None,
                       m: int | None = None, adv_moments=None, mu_old=None, mu_out=None, logp_out=None, ctrl=None):
    """cf2_ppo_policy_grad on torch buffers (include/cf2sim.h describes every argument).  flat: the
    block of ``pack_policy_weights``; idx: int32 row indices; m: rows to use (default: len(idx) or n);
    grad=None evaluates only.  ctrl: the four-word int32 control block of ``adam_step_device``; given,
    the call goes through cf2_ppo_policy_grad_gated and writes nothing once ctrl[0] is set.
    Returns ``summary`` (on the device; nothing synchronises)."""
    from . import _native
    from .vec_env import _check_buf
    lib = _native.load()
    n = obs.shape[0]
    m = int(m) if m is not None else (idx.shape[0] if idx is not None else n)
    d, dev = _check_common(lib, flat, obs, n, idx, m, grad, summary, scratch)
    f32 = torch.float32
    _check_buf(act, "act", (n, 4), f32, dev, align=16)
    _check_buf(logp_old, "logp_old", (n,), f32, dev)
    _check_buf(adv, "adv", (n,), f32, dev)
    _check_buf(adv_moments, "adv_moments", (2,), torch.float64, dev, align=8)
    _check_buf(mu_old, "mu_old", (n, 4), f32, dev)
    _check_buf(mu_out, "mu_out", (m, 4), f32, dev)
    _check_buf(logp_out, "logp_out", (m,), f32, dev)
    _check_buf(ctrl, "ctrl", (4,), torch.int32, dev)
    p = _native.ptr
    args = (p(flat), d, p(obs), p(act), p(logp_old), p(adv), n, p(idx), m, p(adv_moments), float(clip_ratio), p(mu_old),
            p(mu_out), p(logp_out), p(grad), p(summary), p(scratch))
    stream = torch.cuda.current_stream(dev).cuda_stream
    if ctrl is None:
        _native.check(lib.cf2_ppo_policy_grad(*args, stream), "cf2_ppo_policy_grad")
    else:
        _native.check(lib.cf2_ppo_policy_grad_gated(*args, p(ctrl), stream), "cf2_ppo_policy_grad_gated")
    return summary


def value_grad_device(flat, obs, target, summary, scratch, grad=None, idx=None, m: int | None = None, val_out=None):
    """cf2_ppo_value_grad on torch buffers; arguments as ``policy_grad_device``."""
    from . import _native
    from .vec_env import _check_buf
    lib = _native.load()
    n = obs.shape[0]
    m = int(m) if m is not None else (idx.shape[0] if idx is not None else n)
    d, dev = _check_common(lib, flat, obs, n, idx, m, grad, summary, scratch)
    _check_buf(target, "target", (n,), torch.float32, dev)
    _check_buf(val_out, "val_out", (m,), torch.float32, dev)
    p = _native.ptr
    _native.check(lib.cf2_ppo_value_grad(
        p(flat), d, p(obs), p(target), n, p(idx), m, p(val_out), p(grad), p(summary), p(scratch),
        torch.cuda.current_stream(dev).cuda_stream), "cf2_ppo_value_grad")
    return summary


def adam_step_device(flat, grad, exp_avg, exp_avg_sq, begin: int, count: int, step, lr: float, beta1: float = 0.9,
                     beta2: float = 0.999, eps: float = 1e-8, max_grad_norm: float = 0.0, norm_out=None,
                     kl_summary=None, target_kl: float = 0.0, ctrl=None):
    """cf2_adam_step on torch buffers (include/cf2sim.h describes every argument): one Adam step,
    preceded by gradient-norm clipping when max_grad_norm > 0, on the words [begin, begin + count) of
    the flat block.  flat, grad, exp_avg, exp_avg_sq: float32 blocks of the same length; step: int32
    [1]; norm_out: float64 [1]; kl_summary: the float64 [8] summary of a policy call; ctrl: int32 [4],
    zeroed by the caller when an update starts.  Nothing synchronises."""
    from . import _native
    from .vec_env import _check_buf
    lib = _native.load()
    if not isinstance(flat, torch.Tensor) or flat.dim() != 1 or flat.device.type != "cuda":
        raise ValueError("flat must be a 1-d tensor on the GPU")
    dev, f32, words = flat.device, torch.float32, flat.numel()
    begin, count = int(begin), int(count)
    if begin < 0 or count < 0 or begin + count > words:
        raise ValueError(f"the slice [{begin}, {begin + count}) does not lie in a block of {words} words")
    for t, name in ((flat, "flat"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        if t is None:
            raise ValueError(f"{name} is required")
        _check_buf(t, name, (words,), f32, dev)
    if step is None:
        raise ValueError("step is required")
    _check_buf(step, "step", (1,), torch.int32, dev)
    _check_buf(norm_out, "norm_out", (1,), torch.float64, dev, align=8)
    _check_buf(kl_summary, "kl_summary", (8,), torch.float64, dev, align=8)
    _check_buf(ctrl, "ctrl", (4,), torch.int32, dev)
    p = _native.ptr
    _native.check(lib.cf2_adam_step(
        p(flat), p(grad), p(exp_avg), p(exp_avg_sq), begin, count, p(step), float(lr), float(beta1), float(beta2),
        float(eps), float(max_grad_norm), p(norm_out), p(kl_summary), float(target_kl), p(ctrl),
        torch.cuda.current_stream(dev).cuda_stream), "cf2_adam_step")


class DeviceAdam:
    """torch.optim.Adam (defaults: no amsgrad, no weight decay) with optional gradient-norm clipping
    on one slice [begin, begin + size) of a flat weight block of ``count`` words, stepped by
    cf2_adam_step.  Owns exp_avg and exp_avg_sq (whole blocks; only the slice is ever touched), the
    step word and ``norm``, the pre-clip gradient norm of the last applied step.  Everything lives on
    the device; a step never synchronises."""

    def __init__(self, count: int, begin: int, size: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float | None = None, device="cuda"):
        count, begin, size = int(count), int(begin), int(size)
        if begin < 0 or size < 0 or begin + size > count:
            raise ValueError(f"the slice [{begin}, {begin + size}) does not lie in a block of {count} words")
        if not lr >= 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not eps >= 0.0:
            raise ValueError(f"invalid Adam hyper-parameters lr={lr} betas={betas} eps={eps}")
        self.count, self.begin, self.size = count, begin, size
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        self.exp_avg = torch.zeros(count, device=device)
        self.exp_avg_sq = torch.zeros(count, device=device)
        self.step_count = torch.zeros(1, dtype=torch.int32, device=device)
        self.norm = torch.zeros(1, dtype=torch.float64, device=device)

    def step(self, flat, grad, kl_summary=None, target_kl: float = 0.0, ctrl=None) -> None:
        adam_step_device(flat, grad, self.exp_avg, self.exp_avg_sq, self.begin, self.size, self.step_count, self.lr,
                         self.betas[0], self.betas[1], self.eps, self.max_grad_norm, norm_out=self.norm,
                         kl_summary=kl_summary, target_kl=target_kl, ctrl=ctrl)

    def state_dict(self) -> dict:
        return {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(), "step": self.step_count.clone()}

    def load_state_dict(self, sd: dict) -> None:
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count.copy_(sd["step"])


class PPOUpdater:
    """The reference's ``update`` on a ``Rollout``: advantage moments, ``train_pi_iterations`` full-batch
    policy iterations (gradient -> ``pi_optimizer.step()`` -> KL check, stop once the exact KL to the
    policy before the update exceeds ``target_kl``), then ``train_v_iterations`` passes over a fresh
    permutation of the rows split into ``num_mini_batches`` value mini-batches, then ``fused.sync()``.

    The caller builds the optimisers over ``ac.pi_net.parameters()`` and ``ac.v_net.parameters()``;
    this class fixes no learning rate.  ``device=True``: loss and gradient come from the fused HIP
    kernels (the rollout and ``ac`` live on the GPU); ``device=False``: the same loop through
    ``policy_loss_torch`` / ``value_loss_torch`` and autograd, on any device.  ``generator``: the
    torch.Generator of the value passes' permutations (default: the global one of the rollout's
    device).  Scratch, gradient and index buffers are allocated once and re-used while the rollout's
    shape stays the same."""

    def __init__(self, ac: MLPActorCritic, pi_optimizer, v_optimizer, clip_ratio: float, target_kl: float,
                 train_pi_iterations: int = 80, train_v_iterations: int = 5, num_mini_batches: int = 16,
                 fused=None, device: bool = True, generator: torch.Generator | None = None):
        if fused is not None and fused.ac is not ac:
            raise ValueError("fused must wrap the same MLPActorCritic")
        if num_mini_batches < 1:
            raise ValueError("num_mini_batches must be at least 1")
        self.ac, self.pi_optimizer, self.v_optimizer = ac, pi_optimizer, v_optimizer
        self.clip_ratio, self.target_kl = float(clip_ratio), float(target_kl)
        self.train_pi_iterations, self.train_v_iterations = int(train_pi_iterations), int(train_v_iterations)
        self.num_mini_batches = int(num_mini_batches)
        self.fused, self.device, self.generator = fused, bool(device), generator
        self._bufs = None

    def value_minibatches(self, n: int, dev) -> list[torch.Tensor]:
        """One value pass: a permutation of the n rows cut into num_mini_batches consecutive pieces
        (sizes differ by at most one; every row is in exactly one)."""
        gen_dev = self.generator.device if self.generator is not None else dev
        perm = torch.randperm(n, generator=self.generator, device=gen_dev).to(dev)
        nb = min(self.num_mini_batches, n)
        return [perm[(k * n) // nb:((k + 1) * n) // nb] for k in range(nb)]

    def _buffers(self, n: int, d: int, dev):
        from . import _native
        key = (n, d, str(dev))
        if self._bufs is None or self._bufs["key"] != key:
            lib = _native.load()
            nbytes = max(lib.cf2_ppo_scratch_bytes(n, d), lib.cf2_column_moments_scratch_bytes(n, 1))
            self._bufs = {
                "key": key,
                "scratch": torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev),
                "grad": torch.zeros(lib.cf2_policy_weights_count(d), device=dev),
                "idx": torch.empty(n, dtype=torch.int32, device=dev),
                "mu_old": torch.empty(n, 4, device=dev),
                "moments": torch.empty(2, dtype=torch.float64, device=dev),
                "summary": torch.empty(8, dtype=torch.float64, device=dev),
            }
        return self._bufs

    def update(self, rollout: Rollout) -> dict:
        d = rollout.obs.shape[-1]
        obs, act = rollout.obs.reshape(-1, d), rollout.act.reshape(-1, 4)
        logp_old, adv, ret = rollout.logp.reshape(-1), rollout.adv.reshape(-1), rollout.ret.reshape(-1)
        n = obs.shape[0]
        if n == 0 or n >= 2 ** 31:
            raise ValueError(f"a rollout of {n} rows cannot be updated from in one call")
        out = self._update_device(obs, act, logp_old, adv, ret) if self.device \
            else self._update_torch(obs, act, logp_old, adv, ret)
        if self.fused is not None:
            self.fused.sync()
        return out

    # ---- the fused kernels
    @torch.no_grad()
    def _update_device(self, obs, act, logp_old, adv, ret) -> dict:
        from . import _native
        ac, c = self.ac, self.clip_ratio
        n, d, dev = obs.shape[0], obs.shape[1], obs.device
        obs, act, logp_old, adv, ret = (t.contiguous() for t in (obs, act, logp_old, adv, ret))
        B = self._buffers(n, d, dev)
        scratch, grad, summary, mu_old, mom = B["scratch"], B["grad"], B["summary"], B["mu_old"], B["moments"]
        lib = _native.load()
        _native.check(lib.cf2_column_moments(adv.data_ptr(), n, 1, mom.data_ptr(), scratch.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream), "cf2_column_moments")
        flat = pack_policy_weights(ac)
        before = policy_grad_device(flat, obs, act, logp_old, adv, c, summary, scratch, adv_moments=mom,
                                    mu_out=mu_old).clone()
        before_v = value_grad_device(flat, obs, ret, summary, scratch).clone()
        kl, clip_frac, stop = 0.0, 0.0, 0
        for i in range(self.train_pi_iterations):
            policy_grad_device(flat, obs, act, logp_old, adv, c, summary, scratch, grad=grad, adv_moments=mom)
            scatter_flat_grad(ac, grad, "pi")
            self.pi_optimizer.step()
            flat = pack_policy_weights(ac)
            s = policy_grad_device(flat, obs, act, logp_old, adv, c, summary, scratch, adv_moments=mom,
                                   mu_old=mu_old).tolist()        # the KL check reads the host, as the reference
            kl, clip_frac, stop = s[4], s[3], i + 1
            if kl > self.target_kl:
                break
        for _ in range(self.train_v_iterations):
            for mb in self.value_minibatches(n, dev):
                idx = B["idx"][:mb.shape[0]]
                idx.copy_(mb)
                value_grad_device(flat, obs, ret, summary, scratch, grad=grad, idx=idx)
                scatter_flat_grad(ac, grad, "v")
                self.v_optimizer.step()
                flat = pack_policy_weights(ac)
        b, bv = before.tolist(), before_v.tolist()
        return {"LossPi": b[1], "LossV": bv[1], "KL": kl, "StopIter": stop, "ClipFrac": clip_frac}

    # ---- torch autograd (the fall-back, and the reference of the tests)
    def _update_torch(self, obs, act, logp_old, adv, ret) -> dict:
        ac, c = self.ac, self.clip_ratio
        n, dev = obs.shape[0], obs.device
        with torch.no_grad():
            a64 = adv.double()
            mean = a64.mean()
            std = torch.sqrt(((a64 - mean) ** 2).sum() / n)
            adv = ((a64 - mean) / (std + 1e-8)).to(obs.dtype)
            t = policy_terms_torch(ac, obs, act, logp_old, adv, c)
            mu_old, loss_pi = t["mu"], float(t["rows"].double().mean())
            loss_v = float(value_loss_torch(ac, obs, ret))
        kl, clip_frac, stop = 0.0, 0.0, 0
        for i in range(self.train_pi_iterations):
            self.pi_optimizer.zero_grad()
            policy_loss_torch(ac, obs, act, logp_old, adv, c).backward()
            self.pi_optimizer.step()
            with torch.no_grad():
                t = policy_terms_torch(ac, obs, act, logp_old, adv, c, mu_old=mu_old)
                kl = float(t["kl"].double().mean())
                clip_frac = float(((t["ratio"] - 1.0).abs() > c).double().mean())
            stop = i + 1
            if kl > self.target_kl:
                break
        for _ in range(self.train_v_iterations):
            for mb in self.value_minibatches(n, dev):
                self.v_optimizer.zero_grad()
                value_loss_torch(ac, obs[mb], ret[mb]).backward()
                self.v_optimizer.step()
        return {"LossPi": loss_pi, "LossV": loss_v, "KL": kl, "StopIter": stop, "ClipFrac": clip_frac}


class ResidentPPOUpdater:
    """``PPOUpdater(device=True)`` with the optimiser and the loop control on the device: the flat
    weight block is stepped in place by ``DeviceAdam`` (cf2_adam_step: Adam with the reference's
    gradient-norm clipping), and the KL stop is a flag the Adam launch sets and the gated gradient
    launches read, so ``update`` enqueues a fixed sequence of launches and never waits for the GPU.

    The policy phase makes one pass over the rows per iteration.  The gradient call on the weights
    after step i is also the KL evaluation of step i:

        G0   gradient on the starting weights, writes mu_old; its summary is LossPi (its KL is 0)
        A1   Adam                                   (KL 0 <= target_kl: always applied)
        Gi   gated gradient + KL of the weights after step i          i = 1 .. iterations - 1
        A    Adam given Gi's summary: sets the stop flag if KL > target_kl, else applies step i + 1
        E    gated evaluate-only call after the last Adam

    Once the flag is set every later launch returns without writing, so afterwards ``summary`` is the
    evaluation after the last applied step and ctrl[1] is the number of applied steps: the
    reference's rule (step, evaluate, stop if the KL exceeds the target, keep that step).  The
    value phase is ``PPOUpdater``'s: the same mini-batch draws for the same generator, ungated Adam.

    The module stays the source of truth between updates: ``update`` starts from
    ``pack_policy_weights(ac)`` (the current log_std and observation statistics) and ends with
    ``unpack_policy_weights`` and ``fused.sync_from_flat``.  ``update(rollout, read=True)`` reads the
    six results in one transfer at the very end; ``read=False`` returns None without any host
    synchronisation, ``result()`` reads later.  A generator on the rollout's device (or None) keeps
    the permutations on the device too.  ``max_grad_norm``: None or 0 turns clipping off."""

    KEYS = ("LossPi", "LossV", "KL", "ClipFrac", "StopIter", "GradNormPi")

    def __init__(self, ac: MLPActorCritic, pi_lr: float, v_lr: float, clip_ratio: float, target_kl: float,
                 train_pi_iterations: int = 80, train_v_iterations: int = 5, num_mini_batches: int = 16,
                 betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float | None = None, fused=None,
                 generator: torch.Generator | None = None):
        if fused is not None and fused.ac is not ac:
            raise ValueError("fused must wrap the same MLPActorCritic")
        if num_mini_batches < 1:
            raise ValueError("num_mini_batches must be at least 1")
        if target_kl < 0.0:
            raise ValueError("target_kl must not be negative: the first step is taken at KL = 0")
        self.ac, self.fused, self.generator = ac, fused, generator
        self.clip_ratio, self.target_kl = float(clip_ratio), float(target_kl)
        self.train_pi_iterations, self.train_v_iterations = int(train_pi_iterations), int(train_v_iterations)
        self.num_mini_batches = int(num_mini_batches)
        dev = next(ac.parameters()).device
        if dev.type != "cuda":
            raise ValueError("ResidentPPOUpdater needs the module on the GPU")
        count = flat_slice(ac, "v")[1] + 2 * ac.pi_net[0].in_features
        (p0, p1), (v0, v1) = flat_slice(ac, "pi"), flat_slice(ac, "v")
        self.pi_optimizer = DeviceAdam(count, p0, p1 - p0, pi_lr, betas, eps, max_grad_norm, dev)
        self.v_optimizer = DeviceAdam(count, v0, v1 - v0, v_lr, betas, eps, max_grad_norm, dev)
        self.ctrl = torch.zeros(4, dtype=torch.int32, device=dev)
        self.summary0, self.summary, self.summary_v, self.summary_mb = (
            torch.zeros(8, dtype=torch.float64, device=dev) for _ in range(4))
        self.flat = None              # the block the last update stepped
        self._bufs, self._pending = None, None

    value_minibatches = PPOUpdater.value_minibatches
    _buffers = PPOUpdater._buffers

    def state_dict(self) -> dict:
        return {"pi": self.pi_optimizer.state_dict(), "v": self.v_optimizer.state_dict()}

    def load_state_dict(self, sd: dict) -> None:
        self.pi_optimizer.load_state_dict(sd["pi"])
        self.v_optimizer.load_state_dict(sd["v"])

    def result(self) -> dict | None:
        """The last update's results (one device read); None before the first update."""
        if self._pending is None:
            return None
        vals = self._pending.tolist()
        out = dict(zip(self.KEYS, vals))
        out["StopIter"] = int(out["StopIter"])
        return out

    @torch.no_grad()
    def update(self, rollout: Rollout, read: bool = True) -> dict | None:
        from . import _native
        from .rollout import unpack_policy_weights
        ac, c = self.ac, self.clip_ratio
        d = rollout.obs.shape[-1]
        obs, act = rollout.obs.reshape(-1, d).contiguous(), rollout.act.reshape(-1, 4).contiguous()
        logp_old, adv, ret = (t.reshape(-1).contiguous() for t in (rollout.logp, rollout.adv, rollout.ret))
        n, dev = obs.shape[0], obs.device
        if n == 0 or n >= 2 ** 31:
            raise ValueError(f"a rollout of {n} rows cannot be updated from in one call")
        B = self._buffers(n, d, dev)
        scratch, grad, mu_old, mom = B["scratch"], B["grad"], B["mu_old"], B["moments"]
        summary0, summary, ctrl = self.summary0, self.summary, self.ctrl
        lib = _native.load()
        _native.check(lib.cf2_column_moments(adv.data_ptr(), n, 1, mom.data_ptr(), scratch.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream), "cf2_column_moments")
        flat = pack_policy_weights(ac)
        ctrl.zero_()
        summary.zero_()                   # KL and ClipFrac of an update without a policy step
        pol = lambda summ, **kw: policy_grad_device(flat, obs, act, logp_old, adv, c, summ, scratch, adv_moments=mom, **kw)
        value_grad_device(flat, obs, ret, self.summary_v, scratch)
        iters = self.train_pi_iterations
        pol(summary0, mu_out=mu_old, grad=grad if iters > 0 else None)
        if iters > 0:
            self.pi_optimizer.step(flat, grad, kl_summary=summary0, target_kl=self.target_kl, ctrl=ctrl)
            for _ in range(1, iters):
                pol(summary, grad=grad, mu_old=mu_old, ctrl=ctrl)
                self.pi_optimizer.step(flat, grad, kl_summary=summary, target_kl=self.target_kl, ctrl=ctrl)
            pol(summary, mu_old=mu_old, ctrl=ctrl)
        for _ in range(self.train_v_iterations):
            for mb in self.value_minibatches(n, dev):
                idx = B["idx"][:mb.shape[0]]
                idx.copy_(mb)
                value_grad_device(flat, obs, ret, self.summary_mb, scratch, grad=grad, idx=idx)
                self.v_optimizer.step(flat, grad)
        unpack_policy_weights(ac, flat)
        if self.fused is not None:
            self.fused.sync_from_flat(flat)
        self.flat = flat
        self._pending = torch.cat([summary0[1:2], self.summary_v[1:2], summary[4:5], summary[3:4],
                                   ctrl[1:2].double(), self.pi_optimizer.norm])
        return self.result() if read else None


__all__ = ["policy_loss_torch", "policy_terms_torch", "value_loss_torch", "scatter_flat_grad", "flat_slice",
           "policy_grad_device", "value_grad_device", "adam_step_device", "DeviceAdam", "PPOUpdater",
           "ResidentPPOUpdater"]
