"""The PPO update on a batched rollout: the reference's ``update`` --
``train_pi_iterations`` full-batch policy iterations with a KL check after each, then
``train_v_iterations`` passes of ``num_mini_batches`` value mini-batches -- with loss and gradient of
both networks from the fused HIP kernels of csrc/cf2sim_ppo.hip (cf2_ppo_policy_grad,
cf2_ppo_value_grad) and a torch optimiser on the module's parameters.

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
                       m: int | None = None, adv_moments=None, mu_old=None, mu_out=None, logp_out=None):
    """cf2_ppo_policy_grad on torch buffers (include/cf2sim.h describes every argument).  flat: the
    block of ``pack_policy_weights``; idx: int32 row indices; m: rows to use (default: len(idx) or n);
    grad=None evaluates only.  Returns ``summary`` (on the device; nothing synchronises)."""
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
    p = _native.ptr
    _native.check(lib.cf2_ppo_policy_grad(
        p(flat), d, p(obs), p(act), p(logp_old), p(adv), n, p(idx), m, p(adv_moments), float(clip_ratio), p(mu_old),
        p(mu_out), p(logp_out), p(grad), p(summary), p(scratch), torch.cuda.current_stream(dev).cuda_stream),
        "cf2_ppo_policy_grad")
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


__all__ = ["policy_loss_torch", "policy_terms_torch", "value_loss_torch", "scatter_flat_grad", "flat_slice",
           "policy_grad_device", "value_grad_device", "PPOUpdater"]
