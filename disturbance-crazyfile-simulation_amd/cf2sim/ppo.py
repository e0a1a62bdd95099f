"""The PPO update on a batched rollout: the reference's ``update`` --
``train_pi_iterations`` full-batch policy iterations with a KL check after each, then
``train_v_iterations`` passes of ``num_mini_batches`` value mini-batches -- with loss and gradient of
both networks from the fused HIP kernels of csrc/cf2sim_ppo.hip (cf2_ppo_policy_grad,
cf2_ppo_value_grad) and a torch optimiser on the module's parameters (``PPOUpdater``), or with the
optimiser and the KL stop on the device too (``ResidentPPOUpdater``: cf2_adam_step of
csrc/cf2sim_optim.hip on the flat weight block, cf2_ppo_policy_grad_gated).  The second half of the
module is the reference's TRPO and NPG updates (``NaturalGradientUpdater``: cf2_ppo_fisher_vec and the
solver kernels of csrc/cf2sim_natgrad.hip); its header comment restates their rules.  All three
updaters take ``group=``: the ranks of a process group each hold a shard of the rows and update in
lock step from all of them (the reference's ``mpi_avg_grads``; the rank-partial calls, cf2_ppo_reduce
and cf2_moments_combine of csrc/cf2sim_reduce.hip).

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


# ---------------------------------------------------------------------------------------------------
# Data-parallel updates: every gradient, evaluation and Fisher-vector call in two levels.  A rank
# writes a rank-partial block (cf2_ppo_*_partial: its block partials summed in fp64, not divided),
# ``RankReducer.gather`` all-gathers the blocks, and cf2_ppo_reduce sums them in rank order, divides
# by the ranks' row count and rounds once -- on every rank, from the same bits, in the same order.
# grad, summary and with them the KL stop, the CG scalars and the line-search decision are therefore
# the same everywhere, and the weights stay in lock step with no broadcast.
# ---------------------------------------------------------------------------------------------------
def _check_partial(lib, flat, obs, n, idx, m, partial, scratch):
    from .vec_env import _check_buf
    dev, f32 = flat.device, torch.float32
    if dev.type != "cuda":
        raise ValueError("the PPO gradient kernels need buffers on the GPU")
    d = obs.shape[-1] if obs.dim() == 2 else -1
    if d not in (34, 42):
        raise ValueError(f"obs must be [n, 34] or [n, 42], got {tuple(obs.shape)}")
    _check_buf(flat, "flat", (lib.cf2_policy_weights_count(d),), f32, dev)
    _check_buf(obs, "obs", (n, d), f32, dev, align=8)
    if idx is not None:
        _check_buf(idx, "idx", (m,), torch.int32, dev)
    elif m > n:
        raise ValueError(f"m = {m} rows of n = {n} need idx")
    if partial is None:
        raise ValueError("partial is required")
    _check_buf(partial, "partial", (lib.cf2_ppo_partial_doubles(d),), torch.float64, dev, align=8)
    need = lib.cf2_ppo_scratch_bytes(m, d)
    if scratch is None or not isinstance(scratch, torch.Tensor) or scratch.device != dev or not scratch.is_contiguous() \
            or scratch.data_ptr() % 8 or scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"scratch must be a contiguous 8-byte aligned tensor of at least {need} bytes on {dev}")
    return d, dev


def policy_partial_device(flat, obs, act, logp_old, adv, clip_ratio: float, partial, scratch, with_grad: bool = True,
                          idx=None, m: int | None = None, adv_moments=None, moments_count=None, mu_old=None, mu_out=None,
                          logp_out=None, ctrl=None):
    """cf2_ppo_policy_partial on torch buffers: ``policy_grad_device`` ending in a rank-partial block
    (float64 [cf2_ppo_partial_doubles(obs_dim)]) instead of grad and summary.  moments_count: float64
    [1] on the device, the rows ``adv_moments`` was taken over (all ranks').  m = 0 is legal."""
    from . import _native
    from .vec_env import _check_buf
    lib = _native.load()
    n = obs.shape[0]
    m = int(m) if m is not None else (idx.shape[0] if idx is not None else n)
    d, dev = _check_partial(lib, flat, obs, n, idx, m, partial, scratch)
    f32 = torch.float32
    _check_buf(act, "act", (n, 4), f32, dev, align=16)
    _check_buf(logp_old, "logp_old", (n,), f32, dev)
    _check_buf(adv, "adv", (n,), f32, dev)
    _check_buf(adv_moments, "adv_moments", (2,), torch.float64, dev, align=8)
    _check_buf(moments_count, "moments_count", (1,), torch.float64, dev, align=8)
    if adv_moments is not None and moments_count is None:
        raise ValueError("adv_moments needs moments_count, the rows they were taken over")
    _check_buf(mu_old, "mu_old", (n, 4), f32, dev)
    _check_buf(mu_out, "mu_out", (m, 4), f32, dev)
    _check_buf(logp_out, "logp_out", (m,), f32, dev)
    _check_buf(ctrl, "ctrl", (4,), torch.int32, dev)
    p = _native.ptr
    _native.check(lib.cf2_ppo_policy_partial(
        p(flat), d, p(obs), p(act), p(logp_old), p(adv), n, p(idx), m, p(adv_moments), p(moments_count), float(clip_ratio),
        p(mu_old), p(mu_out), p(logp_out), int(bool(with_grad)), p(partial), p(scratch), p(ctrl),
        torch.cuda.current_stream(dev).cuda_stream), "cf2_ppo_policy_partial")
    return partial


def value_partial_device(flat, obs, target, partial, scratch, with_grad: bool = True, idx=None, m: int | None = None,
                         val_out=None, ctrl=None):
    """cf2_ppo_value_partial on torch buffers; arguments as ``policy_partial_device``."""
    from . import _native
    from .vec_env import _check_buf
    lib = _native.load()
    n = obs.shape[0]
    m = int(m) if m is not None else (idx.shape[0] if idx is not None else n)
    d, dev = _check_partial(lib, flat, obs, n, idx, m, partial, scratch)
    _check_buf(target, "target", (n,), torch.float32, dev)
    _check_buf(val_out, "val_out", (m,), torch.float32, dev)
    _check_buf(ctrl, "ctrl", (4,), torch.int32, dev)
    p = _native.ptr
    _native.check(lib.cf2_ppo_value_partial(
        p(flat), d, p(obs), p(target), n, p(idx), m, p(val_out), int(bool(with_grad)), p(partial), p(scratch), p(ctrl),
        torch.cuda.current_stream(dev).cuda_stream), "cf2_ppo_value_partial")
    return partial


def fisher_partial_device(flat, obs, vec, partial, scratch, idx=None, m: int | None = None, ctrl=None):
    """cf2_ppo_fisher_partial on torch buffers: ``fisher_vec_device`` ending in a rank-partial block."""
    from . import _native
    from .vec_env import _check_buf
    lib = _native.load()
    n = obs.shape[0]
    m = int(m) if m is not None else (idx.shape[0] if idx is not None else n)
    if vec is None:
        raise ValueError("vec is required")
    d, dev = _check_partial(lib, flat, obs, n, idx, m, partial, scratch)
    _check_buf(vec, "vec", (flat.numel(),), torch.float32, dev)
    _check_buf(ctrl, "ctrl", (4,), torch.int32, dev)
    p = _native.ptr
    _native.check(lib.cf2_ppo_fisher_partial(p(flat), d, p(obs), n, p(idx), m, p(vec), p(partial), p(scratch), p(ctrl),
                                             torch.cuda.current_stream(dev).cuda_stream), "cf2_ppo_fisher_partial")
    return partial


def ppo_reduce_device(blocks, obs_dim: int, which: str, summary, grad=None, ctrl=None):
    """cf2_ppo_reduce on torch buffers: blocks float64 [world, cf2_ppo_partial_doubles(obs_dim)] in rank
    order -> the ``which`` ("pi" or "v") slice of the flat block ``grad`` (None: the summary only) and
    ``summary``, exactly the words the single-rank call writes.  Nothing synchronises."""
    from . import _native
    from .vec_env import _check_buf
    lib = _native.load()
    if which not in ("pi", "v"):
        raise ValueError(f"which must be 'pi' or 'v', got {which!r}")
    P = lib.cf2_ppo_partial_doubles(int(obs_dim))
    if P == 0:
        raise ValueError(f"obs_dim must be 34 or 42, got {obs_dim}")
    if not isinstance(blocks, torch.Tensor) or blocks.dim() != 2 or blocks.shape[0] < 1 or blocks.device.type != "cuda":
        raise ValueError("blocks must be [world, P] on the GPU")
    dev, world = blocks.device, blocks.shape[0]
    _check_buf(blocks, "blocks", (world, P), torch.float64, dev, align=8)
    if summary is None:
        raise ValueError("summary is required")
    _check_buf(summary, "summary", (8,), torch.float64, dev, align=8)
    _check_buf(grad, "grad", (lib.cf2_policy_weights_count(int(obs_dim)),), torch.float32, dev)
    _check_buf(ctrl, "ctrl", (4,), torch.int32, dev)
    p = _native.ptr
    _native.check(lib.cf2_ppo_reduce(p(blocks), world, int(obs_dim), int(which == "v"), p(grad), p(summary), p(ctrl),
                                     torch.cuda.current_stream(dev).cuda_stream), "cf2_ppo_reduce")
    return summary


def moments_partial_device(x, block, scratch):
    """cf2_column_moments_partial on torch buffers: x float32 [rows, D] (or [rows]: D = 1) -> block
    float64 [1 + 2 D] = {rows, mean[D], M2[D]}; rows = 0 writes a zeroed block."""
    from . import _native
    from .vec_env import _check_buf
    lib = _native.load()
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device.type != "cuda" or not x.is_contiguous() \
            or x.dim() not in (1, 2):
        raise ValueError("x must be a contiguous float32 [rows] or [rows, D] tensor on the GPU")
    rows, d = x.shape[0], (1 if x.dim() == 1 else x.shape[1])
    if block is None:
        raise ValueError("block is required")
    _check_buf(block, "block", (1 + 2 * d,), torch.float64, x.device, align=8)
    need = lib.cf2_column_moments_scratch_bytes(rows, d)
    if rows and (scratch is None or scratch.device != x.device or scratch.data_ptr() % 8
                 or scratch.numel() * scratch.element_size() < need):
        raise ValueError(f"scratch needs {need} bytes, 8-byte aligned, on {x.device}")
    _native.check(lib.cf2_column_moments_partial(x.data_ptr() if rows else None, rows, d, block.data_ptr(),
                                                 _native.ptr(scratch), torch.cuda.current_stream(x.device).cuda_stream),
                  "cf2_column_moments_partial")
    return block


def moments_combine_device(blocks, out):
    """cf2_moments_combine on torch buffers: blocks float64 [world, 1 + 2 D] in rank order -> out
    float64 [1 + 2 D] = {count, mean[D], M2[D]} of all ranks' rows."""
    from . import _native
    from .vec_env import _check_buf
    if not isinstance(blocks, torch.Tensor) or blocks.dim() != 2 or blocks.shape[0] < 1 or blocks.shape[1] < 3 \
            or blocks.shape[1] % 2 == 0 or blocks.device.type != "cuda":
        raise ValueError("blocks must be [world, 1 + 2 D] on the GPU")
    dev, world, words = blocks.device, blocks.shape[0], blocks.shape[1]
    _check_buf(blocks, "blocks", (world, words), torch.float64, dev, align=8)
    if out is None:
        raise ValueError("out is required")
    _check_buf(out, "out", (words,), torch.float64, dev, align=8)
    _native.check(_native.load().cf2_moments_combine(blocks.data_ptr(), world, (words - 1) // 2, out.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream), "cf2_moments_combine")
    return out


class _RankCalls:
    """The device calls of an updater with a ``RankReducer``: the signatures of ``policy_grad_device``,
    ``value_grad_device`` and ``fisher_vec_device``, each as partial -> all-gather -> reduce, plus the
    advantage moments of all ranks' rows (``mom``: {count, mean, M2} on the device)."""

    def __init__(self, reducer, d: int, dev):
        from . import _native
        self.reducer, self.d = reducer, d
        f64 = torch.float64
        self.partial = torch.zeros(_native.load().cf2_ppo_partial_doubles(d), dtype=f64, device=dev)
        self.mom_block = torch.zeros(3, dtype=f64, device=dev)
        self.mom = torch.zeros(3, dtype=f64, device=dev)

    def moments(self, adv, scratch):
        moments_partial_device(adv, self.mom_block, scratch)
        moments_combine_device(self.reducer.gather(self.mom_block), self.mom)

    def policy(self, flat, obs, act, logp_old, adv, clip_ratio, summary, scratch, grad=None, mu_old=None, mu_out=None,
               ctrl=None):
        policy_partial_device(flat, obs, act, logp_old, adv, clip_ratio, self.partial, scratch, with_grad=grad is not None,
                              adv_moments=self.mom[1:], moments_count=self.mom[:1], mu_old=mu_old, mu_out=mu_out, ctrl=ctrl)
        return ppo_reduce_device(self.reducer.gather(self.partial), self.d, "pi", summary, grad=grad, ctrl=ctrl)

    def value(self, flat, obs, target, summary, scratch, grad=None, idx=None):
        value_partial_device(flat, obs, target, self.partial, scratch, with_grad=grad is not None, idx=idx)
        return ppo_reduce_device(self.reducer.gather(self.partial), self.d, "v", summary, grad=grad)

    def fisher(self, flat, obs, vec, out, summary, scratch, idx=None):
        fisher_partial_device(flat, obs, vec, self.partial, scratch, idx=idx)
        return ppo_reduce_device(self.reducer.gather(self.partial), self.d, "pi", summary, grad=out)


def _rank_mean_grads(reducer, params, count: int) -> float:
    """The torch paths' ``mpi_avg_grads``: ``.grad`` of params holds the gradient of a *sum* over this
    rank's ``count`` rows; afterwards it holds the gradient of the mean over all ranks' rows (each
    rank's mean weighted by its row count, so ragged shards give the global mean).  One all_reduce;
    returns the ranks' row count."""
    params = list(params)
    flat = torch.cat([p.grad.reshape(-1).double() for p in params] + [torch.tensor([float(count)], dtype=torch.float64,
                                                                                     device=params[0].device)])
    reducer.sum(flat)
    total = float(flat[-1])
    off = 0
    for p in params:
        p.grad.copy_((flat[off:off + p.numel()] / max(total, 1.0)).view_as(p.grad))     # no rows anywhere: zeros
        off += p.numel()
    return total


def _rank_sums(reducer, *values) -> list:
    """Sums over the ranks of a few host scalars, in fp64 (one all_reduce)."""
    t = torch.tensor([float(v) for v in values], dtype=torch.float64)
    reducer.sum(t)
    return t.tolist()


@torch.no_grad()
def _rank_standardized(reducer, adv, dtype):
    """(adv - mean) / (std + 1e-8) with the moments of all ranks' advantages, in fp64 (two all_reduces:
    the mean, then the squares about it); also returns the ranks' row count."""
    a64 = adv.double()
    N, total = _rank_sums(reducer, a64.numel(), a64.sum())
    mean = total / N
    std = (_rank_sums(reducer, ((a64 - mean) ** 2).sum())[0] / N) ** 0.5
    return ((a64 - mean) / (std + 1e-8)).to(dtype), N


def _rank_value_step(reducer, ac, optimizer, params, obs, target, max_grad_norm: float = 0.0) -> None:
    """One value mini-batch step across ranks: the mean squared error over all ranks' rows of the
    piece (this rank's may be empty)."""
    optimizer.zero_grad()
    ((ac.v_net(_standardized(ac, obs)).squeeze(-1) - target) ** 2).sum().backward()
    _rank_mean_grads(reducer, params, obs.shape[0])
    if max_grad_norm > 0.0:
        nn.utils.clip_grad_norm_(params, max_grad_norm)
    optimizer.step()


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
    shape stays the same.

    ``group``: a torch.distributed process group (or a ``cf2sim.dist.RankReducer``) whose ranks each
    hold a shard of the rows and an identical copy of the module and the optimisers.  Every loss,
    gradient and logged value is then the mean over all ranks' rows (the reference's ``mpi_avg_grads``
    / ``mpi_avg``): on the device path through the rank-partial calls and cf2_ppo_reduce, on the torch
    path through ``all_reduce`` with each rank's mean weighted by its row count.  Every rank permutes
    its own rows with its own generator and mini-batch j of all ranks is one step, as in the
    reference; a pass has ``num_mini_batches`` steps on every rank, some of a rank's pieces empty if it
    has fewer rows.  All ranks compute the same bits, so the modules stay equal without a broadcast.
    None (the default): one rank, today's calls."""

    def __init__(self, ac: MLPActorCritic, pi_optimizer, v_optimizer, clip_ratio: float, target_kl: float,
                 train_pi_iterations: int = 80, train_v_iterations: int = 5, num_mini_batches: int = 16,
                 fused=None, device: bool = True, generator: torch.Generator | None = None, group=None):
        if fused is not None and fused.ac is not ac:
            raise ValueError("fused must wrap the same MLPActorCritic")
        if num_mini_batches < 1:
            raise ValueError("num_mini_batches must be at least 1")
        self.ac, self.pi_optimizer, self.v_optimizer = ac, pi_optimizer, v_optimizer
        self.clip_ratio, self.target_kl = float(clip_ratio), float(target_kl)
        self.train_pi_iterations, self.train_v_iterations = int(train_pi_iterations), int(train_v_iterations)
        self.num_mini_batches = int(num_mini_batches)
        self.fused, self.device, self.generator = fused, bool(device), generator
        from .dist import RankReducer
        self.reducer = RankReducer.of(group)
        self._bufs = None

    def value_minibatches(self, n: int, dev) -> list[torch.Tensor]:
        """One value pass: a permutation of the n rows cut into num_mini_batches consecutive pieces
        (sizes differ by at most one; every row is in exactly one).  Across ranks every rank cuts
        num_mini_batches pieces, empty ones included, so that all ranks take the same number of steps."""
        gen_dev = self.generator.device if self.generator is not None else dev
        perm = torch.randperm(n, generator=self.generator, device=gen_dev).to(dev)
        nb = self.num_mini_batches if self.reducer.active else min(self.num_mini_batches, n)
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
            if self.reducer.active:
                self._bufs["calls"] = _RankCalls(self.reducer, d, dev)
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
        if self.reducer.active:
            R = B["calls"]
            R.moments(adv, scratch)
            pol = lambda flat, **kw: R.policy(flat, obs, act, logp_old, adv, c, summary, scratch, **kw)
            val = lambda flat, **kw: R.value(flat, obs, ret, summary, scratch, **kw)
        else:
            lib = _native.load()
            _native.check(lib.cf2_column_moments(adv.data_ptr(), n, 1, mom.data_ptr(), scratch.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "cf2_column_moments")
            pol = lambda flat, **kw: policy_grad_device(flat, obs, act, logp_old, adv, c, summary, scratch, adv_moments=mom,
                                                        **kw)
            val = lambda flat, **kw: value_grad_device(flat, obs, ret, summary, scratch, **kw)
        flat = pack_policy_weights(ac)
        before = pol(flat, mu_out=mu_old).clone()
        before_v = val(flat).clone()
        kl, clip_frac, stop = 0.0, 0.0, 0
        for i in range(self.train_pi_iterations):
            pol(flat, grad=grad)
            scatter_flat_grad(ac, grad, "pi")
            self.pi_optimizer.step()
            flat = pack_policy_weights(ac)
            s = pol(flat, mu_old=mu_old).tolist()                 # the KL check reads the host, as the reference
            kl, clip_frac, stop = s[4], s[3], i + 1
            if kl > self.target_kl:
                break
        for _ in range(self.train_v_iterations):
            for mb in self.value_minibatches(n, dev):
                idx = B["idx"][:mb.shape[0]]
                idx.copy_(mb)
                val(flat, grad=grad, idx=idx)
                scatter_flat_grad(ac, grad, "v")
                self.v_optimizer.step()
                flat = pack_policy_weights(ac)
        b, bv = before.tolist(), before_v.tolist()
        return {"LossPi": b[1], "LossV": bv[1], "KL": kl, "StopIter": stop, "ClipFrac": clip_frac}

    # ---- torch autograd (the fall-back, and the reference of the tests)
    def _update_torch(self, obs, act, logp_old, adv, ret) -> dict:
        if self.reducer.active:
            return self._update_torch_ranks(obs, act, logp_old, adv, ret)
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

    # ---- torch autograd across ranks: sums per rank, one all_reduce, divided by the ranks' rows
    def _update_torch_ranks(self, obs, act, logp_old, adv, ret) -> dict:
        ac, c, R = self.ac, self.clip_ratio, self.reducer
        n, dev = obs.shape[0], obs.device
        adv, N = _rank_standardized(R, adv, obs.dtype)
        pi_params, v_params = list(ac.pi_net.parameters()), list(ac.v_net.parameters())
        with torch.no_grad():
            t = policy_terms_torch(ac, obs, act, logp_old, adv, c)
            mu_old = t["mu"]
            sq = (ac.v_net(_standardized(ac, obs)).squeeze(-1) - ret) ** 2
            loss_pi, loss_v = (v / N for v in _rank_sums(R, t["rows"].double().sum(), sq.double().sum()))
        kl, clip_frac, stop = 0.0, 0.0, 0
        for i in range(self.train_pi_iterations):
            self.pi_optimizer.zero_grad()
            policy_terms_torch(ac, obs, act, logp_old, adv, c)["rows"].sum().backward()
            _rank_mean_grads(R, pi_params, n)
            self.pi_optimizer.step()
            with torch.no_grad():
                t = policy_terms_torch(ac, obs, act, logp_old, adv, c, mu_old=mu_old)
                kl, clip_frac = (v / N for v in _rank_sums(R, t["kl"].double().sum(),
                                                           ((t["ratio"] - 1.0).abs() > c).double().sum()))
            stop = i + 1
            if kl > self.target_kl:
                break
        for _ in range(self.train_v_iterations):
            for mb in self.value_minibatches(n, dev):
                _rank_value_step(R, ac, self.v_optimizer, v_params, obs[mb], ret[mb])
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
    the permutations on the device too.  ``max_grad_norm``: None or 0 turns clipping off.

    ``group``: as ``PPOUpdater``'s.  Each gradient and evaluation launch pair becomes rank partial ->
    all-gather -> cf2_ppo_reduce, the advantage moments cf2_column_moments_partial -> all-gather ->
    cf2_moments_combine; the Adam launches then read the same grad and summary on every rank, so the
    KL stop falls at the same step everywhere.  Over nccl ``read=False`` still returns without a host
    read; over gloo every all-gather stages through the host (the rehearsal path).  A mini-batch in
    which no rank has a row (fewer rows in all than ``num_mini_batches``) would step on a stale gradient:
    keep ``num_mini_batches`` at or below the ranks' row count."""

    KEYS = ("LossPi", "LossV", "KL", "ClipFrac", "StopIter", "GradNormPi")

    def __init__(self, ac: MLPActorCritic, pi_lr: float, v_lr: float, clip_ratio: float, target_kl: float,
                 train_pi_iterations: int = 80, train_v_iterations: int = 5, num_mini_batches: int = 16,
                 betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float | None = None, fused=None,
                 generator: torch.Generator | None = None, group=None):
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
        from .dist import RankReducer
        self.reducer = RankReducer.of(group)
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
        if self.reducer.active:
            R = B["calls"]
            R.moments(adv, scratch)
            pol = lambda summ, **kw: R.policy(flat, obs, act, logp_old, adv, c, summ, scratch, **kw)
            val = lambda summ, **kw: R.value(flat, obs, ret, summ, scratch, **kw)
        else:
            lib = _native.load()
            _native.check(lib.cf2_column_moments(adv.data_ptr(), n, 1, mom.data_ptr(), scratch.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "cf2_column_moments")
            pol = lambda summ, **kw: policy_grad_device(flat, obs, act, logp_old, adv, c, summ, scratch, adv_moments=mom,
                                                        **kw)
            val = lambda summ, **kw: value_grad_device(flat, obs, ret, summ, scratch, **kw)
        flat = pack_policy_weights(ac)
        ctrl.zero_()
        summary.zero_()                   # KL and ClipFrac of an update without a policy step
        val(self.summary_v)
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
                val(self.summary_mb, grad=grad, idx=idx)
                self.v_optimizer.step(flat, grad)
        unpack_policy_weights(ac, flat)
        if self.fused is not None:
            self.fused.sync_from_flat(flat)
        self.flat = flat
        self._pending = torch.cat([summary0[1:2], self.summary_v[1:2], summary[4:5], summary[3:4],
                                   ctrl[1:2].double(), self.pi_optimizer.norm])
        return self.result() if read else None


# ---------------------------------------------------------------------------------------------------
# Natural-gradient updates (the reference's algs/npg and algs/trpo)
#
# * ``algs/npg``: g = gradient of the unclipped surrogate -mean(ratio A); x = conjugate gradients
#   (``cg_iters`` steps) on (F + damping I) x = -g, where F v is the Hessian-vector product of the mean
#   KL to the detached policy on every ``fvp_stride``-th row; alpha = sqrt(2 target_kl / (x.Hx + 1e-8));
#   step = alpha x; the parameters move by the full step.
# * ``algs/trpo``: the same direction, then a backtracking line search over step fractions
#   decay^j, j = 0 .. line_search_steps - 1: the first trial with a finite loss, an improvement
#   loss_before - loss >= 0 and KL <= 1.5 target_kl is kept; with none the old parameters come back.
# * The critic is IWPG's ``update_value_net``, as in the PPO update.
#
# For this policy (Gaussian, log_std not trained) KL = sum_k (mu_old_k - mu_k)^2 / (2 sigma_k^2), whose
# Hessian at mu = mu_old is exactly F = (1/m) sum_rows J^T Sigma^-1 J: cf2_ppo_fisher_vec evaluates
# that with one tangent pass and the gradient kernel's backward pass; ``fisher_vec_torch`` is the
# reference's double-backward form.  Vectors are in the flat layout of ``pack_policy_weights``
# (matrices input-major), the policy slice [0, flat_slice(ac, "pi")[1]).
# ---------------------------------------------------------------------------------------------------
NG_STATE_DOUBLES = 16
# include/cf2sim.h CF2_NG_*: the words of ng_state
(NG_RDOTR, NG_CG_STEPS, NG_CG_DONE, NG_XHX, NG_ALPHA, NG_EXPECTED, NG_STEP_FRAC, NG_ACCEPT_STEP, NG_LOSS_BEFORE,
 NG_LOSS_AFTER, NG_KL_AFTER, NG_PDOTZ, NG_BDOTB, NG_RESIDUAL) = range(14)


def pi_flat(ac: MLPActorCritic, tensors=None) -> torch.Tensor:
    """The policy slice of the flat layout from six tensors shaped like ac.pi_net's parameters
    (W1 b1 W2 b2 W3 b3; default: the parameters themselves, detached)."""
    params = [p for m in _linears(ac, "pi") for p in (m.weight, m.bias)]
    tensors = [p.detach() for p in params] if tensors is None else list(tensors)
    return torch.cat([t.t().reshape(-1) if t.dim() == 2 else t.reshape(-1) for t in tensors])


def pi_unflat(ac: MLPActorCritic, vec: torch.Tensor) -> list:
    """The inverse of ``pi_flat``: views of the first words of ``vec`` shaped like the parameters."""
    out, off = [], 0
    for m in _linears(ac, "pi"):
        nw, nb = m.weight.numel(), m.bias.numel()
        out += [vec[off:off + nw].view(m.in_features, m.out_features).t(), vec[off + nw:off + nw + nb]]
        off += nw + nb
    return out


@torch.no_grad()
def set_pi_flat(ac: MLPActorCritic, vec: torch.Tensor) -> None:
    """Copy a flat policy slice into ac.pi_net's parameters."""
    params = [p for m in _linears(ac, "pi") for p in (m.weight, m.bias)]
    for p, src in zip(params, pi_unflat(ac, vec)):
        p.copy_(src)


def fisher_vec_torch(ac: MLPActorCritic, obs, vec) -> torch.Tensor:
    """F vec in the reference's form: the gradient of (grad KL . vec), KL the mean divergence to the
    detached policy on the rows ``obs``, through autograd twice.  vec: a flat policy slice (or a
    longer block whose first words are one); any dtype and device.  Returns the flat policy slice."""
    params = [p for m in _linears(ac, "pi") for p in (m.weight, m.bias)]
    with torch.enable_grad():
        mu = ac.pi_net(_standardized(ac, obs))
        log_std = ac.log_std.detach().to(mu.dtype)
        kl = ((mu.detach() - mu) ** 2 * (0.5 * torch.exp(-2.0 * log_std))).sum(-1).mean()
        grads = torch.autograd.grad(kl, params, create_graph=True)
        gv = sum((g * v.to(g.dtype)).sum() for g, v in zip(grads, pi_unflat(ac, vec.detach())))
        hv = torch.autograd.grad(gv, params)
    return pi_flat(ac, [h.detach() for h in hv])


def cg_init_torch(grad: torch.Tensor) -> dict:
    """cf2_ng_cg_init restated: b = -grad, x = 0, r = p = b, rdotr = b.b.  The state is a dict of
    tensors of grad's dtype (scalars 0-dim) plus the Python values ``done`` and ``steps``."""
    b = -grad.detach()
    bb = torch.dot(b, b)
    return {"b": b, "x": torch.zeros_like(b), "r": b.clone(), "p": b.clone(), "rdotr": bb, "bdotb": bb, "residual": bb,
            "done": False, "steps": 0}


def cg_step_torch(st: dict, z: torch.Tensor, damping: float) -> None:
    """cf2_ng_cg_step restated, given z = F p."""
    if st["done"]:
        return
    zd = z + damping * st["p"]
    alpha = st["rdotr"] / (torch.dot(st["p"], zd) + 1e-6)
    st["x"] = st["x"] + alpha * st["p"]
    st["r"] = st["r"] - alpha * zd
    new = torch.dot(st["r"], st["r"])
    st["steps"] += 1
    st["residual"] = new
    if float(torch.sqrt(new)) < 1e-10:
        st["done"] = True
        return
    st["p"] = st["r"] + new / (st["rdotr"] + 1e-6) * st["p"]
    st["rdotr"] = new


def direction_torch(st: dict, z: torch.Tensor, damping: float, target_kl: float) -> None:
    """cf2_ng_direction restated, given z = F x: xHx, alpha, step and the expected improvement."""
    x = st["x"]
    st["xHx"] = torch.dot(x, z + damping * x)
    st["alpha"] = torch.sqrt(2.0 * target_kl / (st["xHx"] + 1e-8))
    st["step"] = st["alpha"] * x
    st["expected"] = torch.dot(st["b"], st["step"])


def line_search_torch(trial: int, total: int, decay: float, target_kl: float, loss: float, kl: float,
                      loss_before: float) -> tuple:
    """cf2_ng_line_search's decision restated: ("accept", decay^trial), ("retry", decay^(trial + 1))
    or ("restore", 0.0) after the last trial."""
    import math
    if math.isfinite(loss) and loss_before - loss >= 0.0 and kl <= 1.5 * target_kl:
        return "accept", decay ** trial
    if trial + 1 < total:
        return "retry", decay ** (trial + 1)
    return "restore", 0.0


def fisher_vec_device(flat, obs, vec, out, summary, scratch, idx=None, m: int | None = None, ctrl=None):
    """cf2_ppo_fisher_vec on torch buffers (include/cf2sim.h describes every argument): the policy
    slice of ``out`` = F vec on the rows ``idx`` (default: the first m) of ``obs``, no damping.  vec and
    out are float32 blocks as long as ``flat``; summary[1] = vec^T F vec.  Nothing synchronises."""
    from . import _native
    from .vec_env import _check_buf
    lib = _native.load()
    n = obs.shape[0]
    m = int(m) if m is not None else (idx.shape[0] if idx is not None else n)
    if vec is None or out is None:
        raise ValueError("vec and out are required")
    d, dev = _check_common(lib, flat, obs, n, idx, m, out, summary, scratch)
    _check_buf(vec, "vec", (flat.numel(),), torch.float32, dev)
    _check_buf(ctrl, "ctrl", (4,), torch.int32, dev)
    p = _native.ptr
    _native.check(lib.cf2_ppo_fisher_vec(p(flat), d, p(obs), n, p(idx), m, p(vec), p(out), p(summary), p(scratch), p(ctrl),
                                         torch.cuda.current_stream(dev).cuda_stream), "cf2_ppo_fisher_vec")
    return summary


def _check_ng(blocks: dict, begin: int, count: int, ng_state, ctrl, ctrl_required=False):
    from .vec_env import _check_buf
    first = next(iter(blocks.values()))
    if not isinstance(first, torch.Tensor) or first.dim() != 1 or first.device.type != "cuda":
        raise ValueError("the solver kernels need 1-d blocks on the GPU")
    dev, words = first.device, first.numel()
    begin, count = int(begin), int(count)
    if begin < 0 or count < 0 or begin + count > words:
        raise ValueError(f"the slice [{begin}, {begin + count}) does not lie in a block of {words} words")
    for name, t in blocks.items():
        if t is None:
            raise ValueError(f"{name} is required")
        _check_buf(t, name, (words,), torch.float32, dev)
    if ng_state is None:
        raise ValueError("ng_state is required")
    _check_buf(ng_state, "ng_state", (NG_STATE_DOUBLES,), torch.float64, dev, align=8)
    if ctrl is None and ctrl_required:
        raise ValueError("ctrl is required")
    _check_buf(ctrl, "ctrl", (4,), torch.int32, dev)
    return begin, count, torch.cuda.current_stream(dev).cuda_stream


def ng_cg_init_device(grad, b, x, r, p, begin: int, count: int, ng_state, ctrl=None) -> None:
    """cf2_ng_cg_init on torch buffers: float32 blocks of one length, ng_state float64 [16]."""
    from . import _native
    begin, count, stream = _check_ng({"grad": grad, "b": b, "x": x, "r": r, "p": p}, begin, count, ng_state, ctrl)
    q = _native.ptr
    _native.check(_native.load().cf2_ng_cg_init(q(grad), q(b), q(x), q(r), q(p), begin, count, q(ng_state), q(ctrl), stream),
                  "cf2_ng_cg_init")


def ng_cg_step_device(z, x, r, p, begin: int, count: int, damping: float, ng_state, ctrl=None) -> None:
    """cf2_ng_cg_step on torch buffers, given z = F p."""
    from . import _native
    begin, count, stream = _check_ng({"z": z, "x": x, "r": r, "p": p}, begin, count, ng_state, ctrl)
    q = _native.ptr
    _native.check(_native.load().cf2_ng_cg_step(q(z), q(x), q(r), q(p), begin, count, float(damping), q(ng_state), q(ctrl),
                                                stream), "cf2_ng_cg_step")


def ng_direction_device(z, x, b, step, flat, flat_old, begin: int, count: int, damping: float, target_kl: float,
                        ng_state, ctrl=None) -> None:
    """cf2_ng_direction on torch buffers, given z = F x: writes step, flat_old = flat, flat += step."""
    from . import _native
    begin, count, stream = _check_ng({"z": z, "x": x, "b": b, "step": step, "flat": flat, "flat_old": flat_old}, begin,
                                     count, ng_state, ctrl)
    q = _native.ptr
    _native.check(_native.load().cf2_ng_direction(q(z), q(x), q(b), q(step), q(flat), q(flat_old), begin, count,
                                                  float(damping), float(target_kl), q(ng_state), q(ctrl), stream),
                  "cf2_ng_direction")


def ng_line_search_device(flat, flat_old, step, begin: int, count: int, trial: int, total: int, decay: float,
                          target_kl: float, eval_summary, loss_before, ng_state, ctrl) -> None:
    """cf2_ng_line_search on torch buffers: eval_summary float64 [8] (the gated evaluation of trial
    ``trial``), loss_before float64 [1] (e.g. ``summary0[1:2]``), ctrl int32 [4]."""
    from . import _native
    from .vec_env import _check_buf
    begin, count, stream = _check_ng({"flat": flat, "flat_old": flat_old, "step": step}, begin, count, ng_state, ctrl,
                                     ctrl_required=True)
    if eval_summary is None or loss_before is None:
        raise ValueError("eval_summary and loss_before are required")
    _check_buf(eval_summary, "eval_summary", (8,), torch.float64, flat.device, align=8)
    _check_buf(loss_before, "loss_before", (1,), torch.float64, flat.device, align=8)
    q = _native.ptr
    _native.check(_native.load().cf2_ng_line_search(q(flat), q(flat_old), q(step), begin, count, int(trial), int(total),
                                                    float(decay), float(target_kl), q(eval_summary), q(loss_before),
                                                    q(ng_state), q(ctrl), stream), "cf2_ng_line_search")


class NaturalGradientUpdater:
    """The reference's TRPO (``algorithm="trpo"``) and NPG (``"npg"``) updates on a ``Rollout``: the
    policy moves along the conjugate-gradient solution of (F + cg_damping I) x = -g, scaled to the KL
    target; TRPO backtracks over ``line_search_steps`` fractions ``line_search_decay``^j, NPG takes the
    full step.  The critic is ``ResidentPPOUpdater``'s value phase.

    ``device=True`` (the module and the rollout on the GPU): ``update`` enqueues a fixed sequence of
    launches on the flat weight block and never waits for the GPU --

        moments   cf2_column_moments of the advantages
        G0        cf2_ppo_policy_grad with clip_ratio = inf (the unclipped surrogate -mean(ratio A)) on
                  the starting weights: gradient, LossPi, and mu_old
        CG        cf2_ng_cg_init, then cg_iters x (cf2_ppo_fisher_vec of p on every fvp_stride-th row,
                  cf2_ng_cg_step)
        D         cf2_ppo_fisher_vec of x, cf2_ng_direction: the step, and trial 0 in the weights
        TRPO      line_search_steps x (gated evaluation with mu_old, cf2_ng_line_search); the launch
                  that accepts, or that restores the old weights after the last trial, sets the stop
                  flag, and every later pair returns without writing
        NPG       one evaluation, for the log
        value     train_v_iterations passes of num_mini_batches mini-batches, cf2_adam_step (the same
                  permutations as ``PPOUpdater`` for the same generator)

    and ends with ``unpack_policy_weights`` / ``fused.sync_from_flat``.  ``update(rollout, read=True)``
    reads the results in one transfer at the end; ``read=False`` returns None without any host
    synchronisation and ``result()`` reads later.  The policy phase holds no optimiser state;
    ``state_dict`` carries the value optimiser's.

    ``device=False``: the same loop through ``fisher_vec_torch``, the ``*_torch`` restatements of the
    solver rules and ``torch.optim.Adam`` for the critic, in the module's dtype on any device: the
    reference of the tests and the path that runs without a GPU.

    Results: LossPi (before the step), LossV, KL of the kept weights (0 when every trial was
    rejected; ng_state also holds their loss), AcceptanceStep (accepted trial + 1; 0: all rejected; NPG: 1),
    StepFrac, xHx, Alpha, ExpectedImprove, CGResidual (|r| after the last CG step), GradNormPi.

    ``group``: as ``PPOUpdater``'s.  The reference averages the gradient and the Fisher-vector product
    over ranks (``mpi_avg_grads``): here the G0, evaluation and Fisher-vector calls go rank partial ->
    all-gather -> cf2_ppo_reduce (every rank takes every ``fvp_stride``-th of its own rows, as every
    process of the reference does), so ``ng_state`` -- the CG scalars, the step size and the line
    search's decision -- is the same on every rank.  ``device=False`` averages the same quantities
    with ``all_reduce``, each rank weighted by its row count."""

    KEYS = ("LossPi", "LossV", "KL", "AcceptanceStep", "StepFrac", "xHx", "Alpha", "ExpectedImprove", "CGResidual",
            "GradNormPi")

    def __init__(self, ac: MLPActorCritic, v_lr: float, target_kl: float, algorithm: str = "trpo", cg_iters: int = 10,
                 cg_damping: float = 0.1, fvp_stride: int = 4, line_search_steps: int = 25,
                 line_search_decay: float = 0.8, train_v_iterations: int = 5, num_mini_batches: int = 16,
                 betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float | None = None, fused=None,
                 generator: torch.Generator | None = None, device: bool = True, group=None):
        if algorithm not in ("trpo", "npg"):
            raise ValueError(f"algorithm must be 'trpo' or 'npg', got {algorithm!r}")
        if fused is not None and fused.ac is not ac:
            raise ValueError("fused must wrap the same MLPActorCritic")
        if num_mini_batches < 1 or fvp_stride < 1 or cg_iters < 0 or line_search_steps < 1:
            raise ValueError("num_mini_batches, fvp_stride and line_search_steps must be at least 1, cg_iters at least 0")
        if not target_kl >= 0.0 or not cg_damping >= 0.0 or not 0.0 < line_search_decay <= 1.0:
            raise ValueError("target_kl and cg_damping must not be negative, line_search_decay must lie in (0, 1]")
        self.ac, self.fused, self.generator, self.algorithm = ac, fused, generator, algorithm
        self.target_kl, self.cg_iters, self.cg_damping = float(target_kl), int(cg_iters), float(cg_damping)
        self.fvp_stride, self.line_search_steps = int(fvp_stride), int(line_search_steps)
        self.line_search_decay = float(line_search_decay)
        self.train_v_iterations, self.num_mini_batches = int(train_v_iterations), int(num_mini_batches)
        self.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        self.device = bool(device)
        from .dist import RankReducer
        self.reducer = RankReducer.of(group)
        self._bufs, self._pending, self.flat = None, None, None
        dev = next(ac.parameters()).device
        if self.device:
            if dev.type != "cuda":
                raise ValueError("NaturalGradientUpdater(device=True) needs the module on the GPU")
            count = flat_slice(ac, "v")[1] + 2 * ac.pi_net[0].in_features
            v0, v1 = flat_slice(ac, "v")
            self.v_optimizer = DeviceAdam(count, v0, v1 - v0, v_lr, betas, eps, max_grad_norm, dev)
            self.ctrl = torch.zeros(4, dtype=torch.int32, device=dev)
            self.ng_state = torch.zeros(NG_STATE_DOUBLES, dtype=torch.float64, device=dev)
            self.summary0, self.summary, self.summary_v, self.summary_mb, self.summary_f = (
                torch.zeros(8, dtype=torch.float64, device=dev) for _ in range(5))
            self.work = {k: torch.zeros(count, device=dev) for k in ("b", "x", "r", "p", "z", "step", "old")}
        else:
            self.v_optimizer = torch.optim.Adam(ac.v_net.parameters(), lr=v_lr, betas=betas, eps=eps)

    value_minibatches = PPOUpdater.value_minibatches
    _buffers = PPOUpdater._buffers

    def state_dict(self) -> dict:
        return {"v": self.v_optimizer.state_dict()}

    def load_state_dict(self, sd: dict) -> None:
        self.v_optimizer.load_state_dict(sd["v"])

    def result(self) -> dict | None:
        """The last update's results (one device read); None before the first update."""
        if self._pending is None:
            return None
        out = dict(zip(self.KEYS, self._pending.tolist() if isinstance(self._pending, torch.Tensor) else self._pending))
        out["AcceptanceStep"] = int(out["AcceptanceStep"])
        return out

    def update(self, rollout: Rollout, read: bool = True) -> dict | None:
        d = rollout.obs.shape[-1]
        obs, act = rollout.obs.reshape(-1, d), rollout.act.reshape(-1, 4)
        logp_old, adv, ret = rollout.logp.reshape(-1), rollout.adv.reshape(-1), rollout.ret.reshape(-1)
        n = obs.shape[0]
        if n == 0 or n >= 2 ** 31:
            raise ValueError(f"a rollout of {n} rows cannot be updated from in one call")
        if self.device:
            self._update_device(obs, act, logp_old, adv, ret)
        else:
            self._update_torch(obs, act, logp_old, adv, ret)
            if self.fused is not None:
                self.fused.sync()
        return self.result() if read else None

    # ---- the launches
    @torch.no_grad()
    def _update_device(self, obs, act, logp_old, adv, ret) -> None:
        from . import _native
        from .rollout import unpack_policy_weights
        ac, inf, kl_t, damp = self.ac, float("inf"), self.target_kl, self.cg_damping
        obs, act, logp_old, adv, ret = (t.contiguous() for t in (obs, act, logp_old, adv, ret))
        n, d, dev = obs.shape[0], obs.shape[1], obs.device
        B = self._buffers(n, d, dev)
        scratch, grad, mu_old, mom = B["scratch"], B["grad"], B["mu_old"], B["moments"]
        if "fvp_idx" not in B or B["fvp_stride"] != self.fvp_stride:
            B["fvp_idx"] = torch.arange(0, n, self.fvp_stride, dtype=torch.int32, device=dev)
            B["fvp_stride"] = self.fvp_stride
        fidx = B["fvp_idx"]
        summary0, summary, ctrl, st, W = self.summary0, self.summary, self.ctrl, self.ng_state, self.work
        if self.reducer.active:
            R = B["calls"]
            R.moments(adv, scratch)
            pol = lambda summ, **kw: R.policy(flat, obs, act, logp_old, adv, inf, summ, scratch, **kw)
            fvp = lambda vec: R.fisher(flat, obs, vec, W["z"], self.summary_f, scratch, idx=fidx)
            val = lambda summ, **kw: R.value(flat, obs, ret, summ, scratch, **kw)
        else:
            lib = _native.load()
            _native.check(lib.cf2_column_moments(adv.data_ptr(), n, 1, mom.data_ptr(), scratch.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "cf2_column_moments")
            pol = lambda summ, **kw: policy_grad_device(flat, obs, act, logp_old, adv, inf, summ, scratch, adv_moments=mom,
                                                        **kw)
            fvp = lambda vec: fisher_vec_device(flat, obs, vec, W["z"], self.summary_f, scratch, idx=fidx)
            val = lambda summ, **kw: value_grad_device(flat, obs, ret, summ, scratch, **kw)
        flat = pack_policy_weights(ac)
        ctrl.zero_()
        p0, p1 = flat_slice(ac, "pi")
        val(self.summary_v)
        pol(summary0, mu_out=mu_old, grad=grad)
        ng_cg_init_device(grad, W["b"], W["x"], W["r"], W["p"], p0, p1 - p0, st)
        for _ in range(self.cg_iters):
            fvp(W["p"])
            ng_cg_step_device(W["z"], W["x"], W["r"], W["p"], p0, p1 - p0, damp, st)
        fvp(W["x"])
        ng_direction_device(W["z"], W["x"], W["b"], W["step"], flat, W["old"], p0, p1 - p0, damp, kl_t, st)
        if self.algorithm == "trpo":
            for j in range(self.line_search_steps):
                pol(summary, mu_old=mu_old, ctrl=ctrl)
                ng_line_search_device(flat, W["old"], W["step"], p0, p1 - p0, j, self.line_search_steps,
                                      self.line_search_decay, kl_t, summary, summary0[1:2], st, ctrl)
            after = [st[NG_KL_AFTER:NG_KL_AFTER + 1], st[NG_ACCEPT_STEP:NG_ACCEPT_STEP + 1],
                     st[NG_STEP_FRAC:NG_STEP_FRAC + 1]]
        else:
            pol(summary, mu_old=mu_old)
            one = torch.ones(1, dtype=torch.float64, device=dev)
            after = [summary[4:5], one, one]
        for _ in range(self.train_v_iterations):
            for mb in self.value_minibatches(n, dev):
                idx = B["idx"][:mb.shape[0]]
                idx.copy_(mb)
                val(self.summary_mb, grad=grad, idx=idx)
                self.v_optimizer.step(flat, grad)
        unpack_policy_weights(ac, flat)
        if self.fused is not None:
            self.fused.sync_from_flat(flat)
        self.flat = flat
        self._pending = torch.cat([summary0[1:2], self.summary_v[1:2], after[0], after[1], after[2], st[NG_XHX:NG_XHX + 1],
                                   st[NG_ALPHA:NG_ALPHA + 1], st[NG_EXPECTED:NG_EXPECTED + 1],
                                   st[NG_RESIDUAL:NG_RESIDUAL + 1].sqrt(), st[NG_BDOTB:NG_BDOTB + 1].sqrt()])

    # ---- torch autograd (the fall-back, and the reference of the tests)
    def _update_torch(self, obs, act, logp_old, adv, ret) -> None:
        ac, inf, kl_t, damp, R = self.ac, float("inf"), self.target_kl, self.cg_damping, self.reducer
        n, dev = obs.shape[0], obs.device
        params = [p for m in _linears(ac, "pi") for p in (m.weight, m.bias)]
        sub = obs[::self.fvp_stride]
        if R.active:
            # sums per rank, one all_reduce each, divided by the ranks' rows
            adv, N = _rank_standardized(R, adv, obs.dtype)
            v_params = list(ac.v_net.parameters())
            with torch.no_grad():
                mu_old = policy_terms_torch(ac, obs, act, logp_old, adv, inf)["mu"]
                sq = (ac.v_net(_standardized(ac, obs)).squeeze(-1) - ret) ** 2
                loss_v = _rank_sums(R, sq.double().sum())[0] / N

            def evaluate():
                with torch.no_grad():
                    t = policy_terms_torch(ac, obs, act, logp_old, adv, inf, mu_old=mu_old)
                    return tuple(v / N for v in _rank_sums(R, t["rows"].double().sum(), t["kl"].double().sum()))

            def rank_mean(vec, count):
                both = torch.cat([vec.double() * count, torch.tensor([float(count)], dtype=torch.float64, device=vec.device)])
                R.sum(both)
                return (both[:-1] / both[-1]).to(vec.dtype)

            rows = policy_terms_torch(ac, obs, act, logp_old, adv, inf)["rows"]
            g = rank_mean(pi_flat(ac, torch.autograd.grad(rows.mean(), params)), n)
            loss_before = _rank_sums(R, rows.detach().double().sum())[0] / N
            fvp = lambda vec: rank_mean(fisher_vec_torch(ac, sub, vec), sub.shape[0])
        else:
            with torch.no_grad():
                a64 = adv.double()
                mean = a64.mean()
                std = torch.sqrt(((a64 - mean) ** 2).sum() / n)
                adv = ((a64 - mean) / (std + 1e-8)).to(obs.dtype)
                mu_old = policy_terms_torch(ac, obs, act, logp_old, adv, inf)["mu"]
                loss_v = float(value_loss_torch(ac, obs, ret))

            def evaluate():
                with torch.no_grad():
                    t = policy_terms_torch(ac, obs, act, logp_old, adv, inf, mu_old=mu_old)
                    return float(t["rows"].double().mean()), float(t["kl"].double().mean())

            rows = policy_terms_torch(ac, obs, act, logp_old, adv, inf)["rows"]
            g = pi_flat(ac, torch.autograd.grad(rows.mean(), params))
            loss_before = float(rows.detach().double().mean())
            fvp = lambda vec: fisher_vec_torch(ac, sub, vec)
        st = cg_init_torch(g)
        for _ in range(self.cg_iters):
            cg_step_torch(st, fvp(st["p"]), damp)
        direction_torch(st, fvp(st["x"]), damp, kl_t)
        theta_old = pi_flat(ac).clone()
        set_pi_flat(ac, theta_old + st["step"])
        if self.algorithm == "trpo":
            total, decay = self.line_search_steps, self.line_search_decay
            for j in range(total):
                loss_j, kl_j = evaluate()
                what, frac = line_search_torch(j, total, decay, kl_t, loss_j, kl_j, loss_before)
                if what == "accept":
                    after = (kl_j, j + 1, frac)
                    break
                if what == "retry":
                    set_pi_flat(ac, theta_old + frac * st["step"])
                else:
                    set_pi_flat(ac, theta_old)
                    after = (0.0, 0, 0.0)
        else:
            loss_j, kl_j = evaluate()
            after = (kl_j, 1, 1.0)
        for _ in range(self.train_v_iterations):
            for mb in self.value_minibatches(n, dev):
                if R.active:
                    _rank_value_step(R, ac, self.v_optimizer, v_params, obs[mb], ret[mb], self.max_grad_norm)
                    continue
                self.v_optimizer.zero_grad()
                value_loss_torch(ac, obs[mb], ret[mb]).backward()
                if self.max_grad_norm > 0.0:
                    nn.utils.clip_grad_norm_(ac.v_net.parameters(), self.max_grad_norm)
                self.v_optimizer.step()
        self._pending = [loss_before, loss_v, after[0], after[1], after[2], float(st["xHx"]), float(st["alpha"]),
                         float(st["expected"]), float(torch.sqrt(st["residual"])), float(torch.sqrt(st["bdotb"]))]


__all__ = ["policy_loss_torch", "policy_terms_torch", "value_loss_torch", "scatter_flat_grad", "flat_slice",
           "policy_grad_device", "value_grad_device", "adam_step_device", "DeviceAdam", "PPOUpdater",
           "ResidentPPOUpdater", "pi_flat", "pi_unflat", "set_pi_flat", "fisher_vec_torch", "cg_init_torch",
           "cg_step_torch", "direction_torch", "line_search_torch", "fisher_vec_device", "ng_cg_init_device",
           "ng_cg_step_device", "ng_direction_device", "ng_line_search_device", "NaturalGradientUpdater", "policy_partial_device",
           "value_partial_device", "fisher_partial_device", "ppo_reduce_device", "moments_partial_device",
           "moments_combine_device"]
