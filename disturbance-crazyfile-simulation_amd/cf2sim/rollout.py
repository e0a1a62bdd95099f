"""Batched rollout caller: the reference's PPO/IWPG data collection
with every env of a GPU stepped at once instead of one env per MPI process.

Reference behaviour restated (paths relative to phoenix_drone_simulation/):

* ``ActorCritic`` (algs/core.py:300-395) with ``MLPGaussianActor`` (core.py:228-291) and
  ``MLPCritic``; PPO defaults (algs/ppo/defaults.py:8-17): pi 34->50->50->4 ReLU with a fixed
  log_std = log(0.5) (annealed by ``set_log_std``), v 34->64->64->1 tanh, gamma 0.99,
  lam 0.95 (algs/iwpg/iwpg.py:40), Linear layers, identity output.
* ``IWPGAlgorithm.roll_out`` (algs/iwpg/iwpg.py:372-410): step the policy, store
  (obs, act, rew, val, logp), and at an episode end call ``finish_path(last_val)`` with
  last_val = 0 on a terminal state and V(s) on a time-out or at the end of the epoch.
* ``finish_path`` / ``calculate_adv_and_value_targets`` (algs/core.py:459-535): GAE
  A_t = sum_k (gamma*lam)^k delta_{t+k}, delta_t = r_t + gamma V_{t+1} - V_t, value targets
  A_t + V_t, over each episode slice; with reward scaling (IWPG default use_reward_scaling=True,
  algs/iwpg/iwpg.py:56) the rewards entering delta are clip(r / (ret_std + 1e-5), -10, 10)
  (core.py:522-529) and the unscaled discounted returns feed the return statistics.
* Observation standardisation (IWPG default use_standardized_obs=True, iwpg.py:59):
  ``ActorCritic.step`` feeds (obs - mean) / (std + 1e-5) to both networks (core.py:383-388);
  the statistics are ``OnlineMeanStd`` (utils/online_mean_std.py), updated once per epoch by
  ``update_running_statistics`` (iwpg.py:412-420).  The fused kernel standardises the observation
  in registers before the first layer (pack_policy_weights carries mean and 1 / (std + eps)).
  ``update_running_statistics(..., device=True)`` takes the batch moments from one pass of a HIP
  kernel over the rollout (cf2_column_moments) instead of torch's passes.
* The epoch log's EpRet / EpLen / EpCosts (``logger.store`` at every episode end in roll_out):
  ``EpisodeStats``, per-env running sums carried across collects and reduced on the device
  (cf2_episode_stats).

Here N envs run in lock step with on-device auto-reset, so episode boundaries differ per env.
``gae`` evaluates the same recursion over a [T, N] buffer with per-env masks:
terminal -> bootstrap 0; truncated (TimeLimit) -> bootstrap V(final_obs), the pre-reset
observation the env reports; end of the buffer -> V(obs_T).  This equals running the reference's
finish_path on every env's episode slices (tests/test_rollout.py checks exactly that).
One edge differs: roll_out tests its own ``ep_len == max_ep_len`` and so bootstraps a terminal
state reached exactly at the time limit; gym's TimeLimit (and this env) reports that step as
terminal, not truncated, and it bootstraps 0.
"""
from __future__ import annotations

import dataclasses
import math

import torch
from torch import nn


def _mlp(sizes, activation, output_activation=nn.Identity):
    layers = []
    for j in range(len(sizes) - 1):
        act = activation if j < len(sizes) - 2 else output_activation
        layers += [nn.Linear(sizes[j], sizes[j + 1]), act()]
    return nn.Sequential(*layers)


_ACT = {"relu": nn.ReLU, "tanh": nn.Tanh, "identity": nn.Identity}


class OnlineMeanStd(nn.Module):
    """Running mean / standard deviation (utils/online_mean_std.py): the incremental update of
    Chan et al. over batches.  ``update`` / ``update_device`` with ``group=`` first combine the ranks'
    batch moments (the reference's MPI averages), so every rank carries the same statistics.

    Provenance: this restates the reference's OnlineMeanStd closely -- same epsilon, same clip
    bound 10, the same n_A / n_AB / delta / mean / M2 update in the same order -- because the
    standardised observations must reproduce the reference's arithmetic to match
    tests/golden/golden_f3.npz (generated from the reference's own class).  It is a ~35-line
    standard algorithm, not new design."""

    def __init__(self, epsilon: float = 1e-5, shape=()):
        super().__init__()
        self.register_buffer("mean", torch.zeros(*shape))
        self.register_buffer("std", torch.ones(*shape))
        self.register_buffer("count", torch.zeros(1))
        self.eps = epsilon
        self.bound = 10
        self.shape = tuple(shape)

    def forward(self, x, subtract_mean: bool = True, clip: bool = False):
        x_new = (x - self.mean) / (self.std + self.eps) if subtract_mean else x / (self.std + self.eps)
        return torch.clamp(x_new, -self.bound, self.bound) if clip else x_new

    def std_host(self) -> float:
        """std as a host float (shape (1,) statistics), re-read from the device only after the
        buffer changed (in place or replaced): collect() needs it every epoch for reward scaling,
        and a device read would drain the GPU's queue at the start of every collect."""
        t = self.std
        if getattr(self, "_std_host_key", None) is None or self._std_host_key[0] is not t \
                or self._std_host_key[1] != t._version:
            self._std_host = float(t.item())
            self._std_host_key = (t, t._version)
        return self._std_host

    @torch.no_grad()
    def update(self, x: torch.Tensor, group=None) -> None:
        """One batch.  ``group`` (a process group or a ``cf2sim.dist.RankReducer``): the batch is the
        ranks' batches together -- their moments are combined by ``rank_moments_torch`` and go through
        ``update_from_moments``, so every rank ends with the same bits."""
        x = torch.as_tensor(x, dtype=torch.float32, device=self.mean.device)
        if self.shape[0] == 1:
            if x.dim() != 1:
                raise ValueError(f"expected a 1-d batch, got {tuple(x.shape)}")
            x = x.view(-1, 1)
        elif x.dim() != 2 or x.shape[1] != self.shape[0]:
            raise ValueError(f"expected [B, {self.shape[0]}], got {tuple(x.shape)}")
        from .dist import RankReducer
        if RankReducer.of(group).active:
            self.update_from_moments(*rank_moments_torch(x, group))
            return
        n_b = x.shape[0]
        n_a = self.count.clone()
        n_ab = self.count + n_b
        delta = x.mean(dim=0) - self.mean
        mean_new = self.mean + delta * n_b / n_ab
        batch_var = torch.mean((x - mean_new) ** 2, dim=0)
        m2_ab = n_a * torch.square(self.std) + n_b * batch_var + delta ** 2 * (n_a * n_b / n_ab)
        self.mean.copy_(mean_new)
        self.count.copy_(n_ab)
        self.std.copy_(torch.sqrt(m2_ab / n_ab))

    @torch.no_grad()
    def update_from_moments(self, n_b: int, mean_b: torch.Tensor, m2_b: torch.Tensor) -> None:
        """``update`` from a batch's moments instead of its rows: n_b rows with column means mean_b
        and M2_b = sum (x - mean_b)^2.  Same arithmetic, including update's batch variance about the
        *new* mean (the part golden_f3.npz pins), which from moments is
        (M2_b + n_b (mean_b - mean_new)^2) / n_b.  n_b may be a one-element float64 tensor on the
        statistics' device (the ranks' row count from cf2_moments_combine; it is not checked, so that
        nothing waits for it).  Evaluated in fp64 (count read into fp64; the fp32
        count buffer alone would stop counting single rows at 2^24) and rounded once into the fp32
        buffers; no host synchronisation."""
        dev = self.mean.device
        mean_b = torch.as_tensor(mean_b, dtype=torch.float64, device=dev).reshape(self.shape)
        m2_b = torch.as_tensor(m2_b, dtype=torch.float64, device=dev).reshape(self.shape)
        if isinstance(n_b, torch.Tensor):
            n_b = n_b.to(device=dev, dtype=torch.float64).reshape(())
        else:
            n_b = int(n_b)
            if n_b <= 0:
                raise ValueError(f"a batch has at least one row, got {n_b}")
        n_a = self.count.double()
        n_ab = n_a + n_b
        mean_a = self.mean.double()
        delta = mean_b - mean_a
        mean_new = mean_a + delta * n_b / n_ab
        batch_var = (m2_b + n_b * torch.square(mean_b - mean_new)) / n_b
        m2_ab = n_a * torch.square(self.std.double()) + n_b * batch_var + delta ** 2 * (n_a * n_b / n_ab)
        self.mean.copy_(mean_new)
        self.count.copy_(n_ab)
        self.std.copy_(torch.sqrt(m2_ab / n_ab))

    @torch.no_grad()
    def update_device(self, x: torch.Tensor, group=None) -> None:
        """``update(x)`` for a float32 batch on the GPU in one pass over x: cf2_column_moments
        (fp64 column means and M2, csrc/cf2sim_stats.hip), then ``update_from_moments``.  x is
        [B, D] (or [B] for shape (1,) statistics), contiguous; nothing synchronises with the host.
        ``group``: the ranks' moments blocks (cf2_column_moments_partial) are all-gathered and folded
        in rank order by cf2_moments_combine first, the same bits on every rank; a rank may have no
        row.  Over gloo the all-gather stages through the host."""
        from . import _native
        dev = self.mean.device
        d = self.shape[0]
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != dev or not x.is_contiguous():
            raise ValueError(f"update_device needs a contiguous float32 tensor on {dev}")
        if (x.dim() != 1) if d == 1 else (x.dim() != 2 or x.shape[1] != d):
            raise ValueError(f"expected {'[B]' if d == 1 else f'[B, {d}]'}, got {tuple(x.shape)}")
        rows = x.shape[0]
        from .dist import RankReducer
        reducer = RankReducer.of(group)
        if reducer.active:
            from .ppo import moments_combine_device, moments_partial_device
            lib = _native.load()
            need = lib.cf2_column_moments_scratch_bytes(max(rows, 1), d)
            buf = getattr(self, "_rank_moments_buf", None)
            if buf is None or buf[0].device != dev or buf[0].numel() * 8 < need:
                buf = (torch.empty((need + 7) // 8, dtype=torch.float64, device=dev),
                       torch.empty(1 + 2 * d, dtype=torch.float64, device=dev),
                       torch.empty(1 + 2 * d, dtype=torch.float64, device=dev))
                self._rank_moments_buf = buf
            scratch, block, out = buf
            moments_partial_device(x, block, scratch)
            moments_combine_device(reducer.gather(block), out)
            self.update_from_moments(out[:1], out[1:1 + d], out[1 + d:])
            return
        if rows == 0:
            raise ValueError("a batch has at least one row, got 0")
        lib = _native.load()
        need = lib.cf2_column_moments_scratch_bytes(rows, d)
        buf = getattr(self, "_moments_buf", None)
        if buf is None or buf[0].device != dev or buf[0].numel() * 8 < need:
            buf = (torch.empty((need + 7) // 8, dtype=torch.float64, device=dev),
                   torch.empty(2 * d, dtype=torch.float64, device=dev))
            self._moments_buf = buf           # plain attribute: not part of the state dict
        scratch, out = buf
        _native.check(lib.cf2_column_moments(x.data_ptr(), rows, d, out.data_ptr(), scratch.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream), "cf2_column_moments")
        self.update_from_moments(rows, out[:d], out[d:])


class MLPActorCritic(nn.Module):
    """Gaussian MLP policy + MLP value function with the reference's PPO defaults, the
    observation standardisation and the return statistics of reward scaling."""

    def __init__(self, obs_dim: int = 34, act_dim: int = 4, pi_hidden=(50, 50), pi_activation="relu",
                 v_hidden=(64, 64), v_activation="tanh", log_std: float = math.log(0.5),
                 use_standardized_obs: bool = True, use_scaled_rewards: bool = True):
        super().__init__()
        self.pi_net = _mlp([obs_dim, *pi_hidden, act_dim], _ACT[pi_activation])
        self.v_net = _mlp([obs_dim, *v_hidden, 1], _ACT[v_activation])
        self.log_std = nn.Parameter(torch.full((act_dim,), float(log_std)), requires_grad=False)
        self.obs_oms = OnlineMeanStd(shape=(obs_dim,)) if use_standardized_obs else None
        self.ret_oms = OnlineMeanStd(shape=(1,)) if use_scaled_rewards else None

    def load_reference_state_dict(self, sd: dict):
        """Load a state_dict of the reference's ActorCritic (keys pi.net.{0,2,4}.*, pi.log_std,
        v.net.{0,2,4}.*, obs_oms.*, ret_oms.*; algs/core.py:314-364)."""
        def t(k):
            return torch.as_tensor(sd[k], dtype=torch.float32)
        with torch.no_grad():
            for mine, ref in ((self.pi_net, "pi.net"), (self.v_net, "v.net")):
                for i in (0, 2, 4):
                    mine[i].weight.copy_(t(f"{ref}.{i}.weight"))
                    mine[i].bias.copy_(t(f"{ref}.{i}.bias"))
            self.log_std.copy_(t("pi.log_std"))
            for name, oms in (("obs_oms", self.obs_oms), ("ret_oms", self.ret_oms)):
                if oms is not None and f"{name}.mean" in sd:
                    oms.mean.copy_(t(f"{name}.mean")); oms.std.copy_(t(f"{name}.std")); oms.count.copy_(t(f"{name}.count"))

    def normalize(self, obs: torch.Tensor) -> torch.Tensor:
        return self.obs_oms(obs) if self.obs_oms is not None else obs

    def set_log_std(self, frac: float):
        """Exploration-noise annealing of core.py:274-281 (std 0.5 -> 0.01 as frac goes 1 -> 0)."""
        assert 0.0 <= frac <= 1.0
        with torch.no_grad():
            self.log_std.fill_(math.log(0.499 * frac + 0.01))

    @torch.no_grad()
    def step(self, obs: torch.Tensor, generator: torch.Generator | None = None, deterministic: bool = False):
        """(action, value, log_prob) for a batch of observations (core.py:371-395)."""
        obs = self.normalize(obs)
        mu = self.pi_net(obs)
        v = self.v_net(obs).squeeze(-1)
        if deterministic:
            return mu, v, torch.ones_like(mu)
        std = self.log_std.exp()
        eps = torch.randn(mu.shape, device=mu.device, dtype=mu.dtype, generator=generator)
        a = mu + std * eps
        # Normal(mu, std).log_prob(a).sum(-1)
        logp = (-0.5 * eps.pow(2) - self.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
        return a, v, logp

    @torch.no_grad()
    def value(self, obs: torch.Tensor) -> torch.Tensor:
        return self.v_net(self.normalize(obs)).squeeze(-1)

    @torch.no_grad()
    def log_prob(self, obs: torch.Tensor, act: torch.Tensor) -> torch.Tensor:
        """Normal(mu(obs), std).log_prob(act).sum(-1) (core.py:253-259)."""
        mu = self.pi_net(self.normalize(obs))
        return torch.distributions.Normal(mu, self.log_std.exp()).log_prob(act).sum(-1)


@torch.no_grad()
def rank_moments_torch(x: torch.Tensor, group) -> tuple:
    """(count, mean[D], M2[D]) of the ranks' [B_r, D] batches together, in fp64: each rank's two-pass
    moments, all-gathered (``RankReducer.gather``) and folded left in rank order with the update of
    Chan et al., batches of no rows skipped -- cf2_moments_combine's arithmetic in torch, for the path
    that runs without a GPU.  Every rank gets the same bits.  count is a Python int."""
    from .dist import RankReducer
    x64 = x.double()
    rows, d = x64.shape
    mean = x64.mean(dim=0) if rows else torch.zeros(d, dtype=torch.float64, device=x.device)
    m2 = ((x64 - mean) ** 2).sum(dim=0)
    block = torch.cat([torch.tensor([float(rows)], dtype=torch.float64, device=x.device), mean, m2])
    blocks = RankReducer.of(group).gather(block).cpu()
    n, mean, m2 = 0.0, None, None
    for b in blocks:
        bn = float(b[0])
        if not bn > 0.0:
            continue
        if n == 0.0:
            n, mean, m2 = bn, b[1:1 + d].clone(), b[1 + d:].clone()
            continue
        nab, delta = n + bn, b[1:1 + d] - mean
        mean = mean + delta * (bn / nab)
        m2 = m2 + b[1 + d:] + delta * delta * (n * bn / nab)
        n = nab
    if n == 0.0:
        raise ValueError("a batch has at least one row on some rank")
    return int(n), mean, m2


def update_running_statistics(ac: MLPActorCritic, rollout: "Rollout", fused: "FusedActorCritic | None" = None,
                              device: bool = False, group=None):
    """IWPGAlgorithm.update_running_statistics (iwpg.py:412-420) on a whole batched rollout: the raw
    observations update the observation statistics, the discounted returns the return statistics.
    A FusedActorCritic over `ac` is re-synced (its weight block carries the standardisation).
    device=True: both updates read the rollout once through cf2_column_moments
    (``OnlineMeanStd.update_device``) instead of torch's passes over it.
    group: a process group (or ``cf2sim.dist.RankReducer``) whose ranks each hold a shard of the envs:
    both updates are from the batch moments of all ranks' rows, so every rank carries the same
    ``obs_oms`` / ``ret_oms`` (the reference's MPI-averaged statistics)."""
    kw = {} if group is None else {"group": group}
    if ac.obs_oms is not None:
        upd = ac.obs_oms.update_device if device else ac.obs_oms.update
        upd(rollout.obs.reshape(-1, rollout.obs.shape[-1]), **kw)
    if ac.ret_oms is not None:
        upd = ac.ret_oms.update_device if device else ac.ret_oms.update
        upd(rollout.discounted_ret.reshape(-1), **kw)
    if fused is not None:
        fused.sync()


def pack_policy_weights(ac: MLPActorCritic) -> torch.Tensor:
    """Flatten an MLPActorCritic with the default shapes into the flat weight block of
    cf2_policy_pack (input-major matrices: pi W1 b1 W2 b2 W3 b3 log_std, then v W1 b1 W2 b2 W3 b3,
    then the observation standardisation mean[D] and scale[D] = 1 / (std + eps), computed in fp64;
    identity without obs_oms).  The kernel standardises the observation before the first layer,
    as ActorCritic.step does (core.py:383-388)."""
    lin_pi = [m for m in ac.pi_net if isinstance(m, nn.Linear)]
    lin_v = [m for m in ac.v_net if isinstance(m, nn.Linear)]
    shapes = [(m.out_features, m.in_features) for m in lin_pi] + [(m.out_features, m.in_features) for m in lin_v]
    d = lin_pi[0].in_features
    if shapes != [(50, d), (50, 50), (4, 50), (64, d), (64, 64), (1, 64)] or d not in (34, 42):
        raise ValueError(f"the fused kernel implements the PPO default networks only, got {shapes}")
    parts = []
    for lins in (lin_pi, lin_v):
        for m in lins:
            parts += [m.weight.detach().t().reshape(-1), m.bias.detach()]
        if lins is lin_pi:
            parts.append(ac.log_std.detach())
    dev = lin_pi[0].weight.device
    if ac.obs_oms is not None:
        parts += [ac.obs_oms.mean.detach(), 1.0 / (ac.obs_oms.std.detach().double() + ac.obs_oms.eps)]
    else:
        parts += [torch.zeros(d, device=dev), torch.ones(d, device=dev)]
    return torch.cat([p.float().reshape(-1) for p in parts]).contiguous()


@torch.no_grad()
def unpack_policy_weights(ac: MLPActorCritic, flat: torch.Tensor) -> None:
    """The inverse of ``pack_policy_weights`` for the twelve Linear tensors (pi W1 b1 W2 b2 W3 b3,
    v likewise): copy them out of a flat block into the module, bit for bit.  ``log_std`` and the
    observation statistics are left alone (the module owns them; the block only carries copies)."""
    lin_pi = [m for m in ac.pi_net if isinstance(m, nn.Linear)]
    lin_v = [m for m in ac.v_net if isinstance(m, nn.Linear)]
    d = lin_pi[0].in_features
    want = sum(m.weight.numel() + m.bias.numel() for m in lin_pi + lin_v) + ac.log_std.numel() + 2 * d
    if flat.dim() != 1 or flat.numel() != want or flat.dtype != torch.float32:
        raise ValueError(f"flat must be a float32 block of {want} words, got {tuple(flat.shape)} {flat.dtype}")
    off = 0
    for lins in (lin_pi, lin_v):
        for m in lins:
            nw, nb = m.weight.numel(), m.bias.numel()
            m.weight.copy_(flat[off:off + nw].view(m.in_features, m.out_features).t())
            m.bias.copy_(flat[off + nw:off + nw + nb])
            off += nw + nb
        if lins is lin_pi:
            off += ac.log_std.numel()


POLICY_PRECISIONS = {"fp32": 0, "bf16x3": 1}     # cf2_policy_precision (include/cf2sim.h)


class FusedActorCritic:
    """``MLPActorCritic.step`` / ``value`` through the fused HIP kernel (cf2_policy_forward).
    Sampling noise comes from Philox keyed (seed, call counter, row): reproducible, independent
    of batch geometry.  Call ``sync()`` after changing the torch module's parameters.

    precision: "fp32" -- exact fp32 products on the matrix cores (the result of an fmaf chain);
    "bf16x3" -- split-bf16 products (x = hi + lo, three bf16 MFMAs): <= ~1.1e-5 relative error
    per product, fp32 accumulation and activations, ~5x the fp32 matrix rate.  The collected
    log-probabilities do not depend on it (logp is a function of the drawn noise only)."""

    def __init__(self, ac: MLPActorCritic, seed: int = 0, precision: str = "bf16x3"):
        from . import _native
        if precision not in POLICY_PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(POLICY_PRECISIONS)}, got {precision!r}")
        self.ac = ac
        self.lib = _native.load()
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counter = 0
        self.precision = precision
        self.prec = POLICY_PRECISIONS[precision]
        self.obs_dim = ac.pi_net[0].in_features
        self.sync()

    def sync(self):
        """Re-pack the weights: the flat block (pack_policy_weights) -> the kernel's MFMA fragment
        block (cf2_policy_pack, one launch)."""
        dev = next(self.ac.parameters()).device
        self.sync_from_flat(pack_policy_weights(self.ac).to(dev))

    def sync_from_flat(self, flat: torch.Tensor):
        """``sync()`` straight from a flat block (the layout of pack_policy_weights) that already
        holds the module's values, e.g. the one a device-side optimiser stepped."""
        from . import _native
        dev = next(self.ac.parameters()).device
        if not isinstance(flat, torch.Tensor) or flat.dtype != torch.float32 or flat.device != dev \
                or not flat.is_contiguous() or flat.numel() != self.lib.cf2_policy_weights_count(self.obs_dim):
            raise ValueError(f"flat must be a contiguous float32 block of "
                             f"{self.lib.cf2_policy_weights_count(self.obs_dim)} words on {dev}")
        self.w = torch.empty(self.lib.cf2_policy_packed_count(self.obs_dim, self.prec), device=dev)
        self.w_ptr = self.w.data_ptr()
        _native.check(self.lib.cf2_policy_pack(flat.data_ptr(), self.obs_dim, self.prec, self.w.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream), "cf2_policy_pack")

    @torch.no_grad()
    def step(self, obs: torch.Tensor, deterministic: bool = False, row_offset: int = 0):
        from . import _native
        n = obs.shape[0]
        obs = obs.contiguous()
        act = torch.empty(n, 4, device=obs.device)
        val = torch.empty(n, device=obs.device)
        logp = torch.empty(n, device=obs.device)
        _native.check(self.lib.cf2_policy_forward(
            self.w.data_ptr(), n, self.obs_dim, self.prec, obs.data_ptr(), self.seed, self.counter & 0xFFFFFFFF, row_offset,
            0 if deterministic else 1, act.data_ptr(), val.data_ptr(), logp.data_ptr(),
            torch.cuda.current_stream(obs.device).cuda_stream), "cf2_policy_forward")
        self.counter += 1
        return act, val, logp

    @torch.no_grad()
    def step_into(self, obs: torch.Tensor, act: torch.Tensor, val: torch.Tensor, logp: torch.Tensor,
                  row_offset: int = 0):
        """step() into caller buffers.  row_offset: global index of row 0 (the sampling noise of row
        r is keyed by row_offset + r; collect() passes the env shard's env_id_offset, so a rank's
        envs draw the noise they would draw in one process holding every env)."""
        from . import _native
        _native.check(self.lib.cf2_policy_forward(
            self.w.data_ptr(), obs.shape[0], self.obs_dim, self.prec, obs.data_ptr(), self.seed,
            self.counter & 0xFFFFFFFF, int(row_offset), 1,
            act.data_ptr(), val.data_ptr(), logp.data_ptr(), torch.cuda.current_stream(obs.device).cuda_stream),
            "cf2_policy_forward")
        self.counter += 1

    @torch.no_grad()
    def value_masked(self, obs: torch.Tensor, mask: torch.Tensor, out: torch.Tensor):
        from . import _native
        _native.check(self.lib.cf2_value_forward_masked(
            self.w.data_ptr(), obs.shape[0], self.obs_dim, self.prec, obs.contiguous().data_ptr(),
            mask.to(torch.uint8).contiguous().data_ptr(), out.data_ptr(),
            torch.cuda.current_stream(obs.device).cuda_stream), "cf2_value_forward_masked")
        return out

    @torch.no_grad()
    def value(self, obs: torch.Tensor) -> torch.Tensor:
        return self.step(obs, deterministic=True)[1]


def gae(rew, val, done, trunc, last_val, trunc_val, gamma: float = 0.99, lam: float = 0.95,
        rew_den: float | None = None, with_discounted: bool = False):
    """Batched GAE over [T, N] buffers with per-env episode boundaries.

    rew, val:   [T, N] rewards r_t and values V(s_t)
    done:       [T, N] bool, episode ended at t (terminal or truncated; the env auto-reset)
    trunc:      [T, N] bool, the end was a TimeLimit truncation (bootstrap from trunc_val)
    last_val:   [N]    V(s_T) of the observation after the last step (epoch cut-off)
    trunc_val:  [T, N] V(final_obs_t) where trunc, anything elsewhere
    rew_den:    reward scaling (core.py:522-529): delta uses clip(r / rew_den, -10, 10) with
                rew_den = ret_oms.std + 1e-5; None = unscaled
    Returns (adv [T, N], value_targets [T, N]) and, with with_discounted, the per-episode
    discounted returns of the unscaled rewards bootstrapped like finish_path (core.py:519)."""
    T = rew.shape[0]
    adv = torch.empty_like(rew)
    disc = torch.empty_like(rew) if with_discounted else None
    nxt_adv = torch.zeros_like(last_val)
    nxt_val = last_val
    nxt_ret = last_val
    for t in range(T - 1, -1, -1):
        d = done[t]
        boot = torch.where(d, torch.where(trunc[t], trunc_val[t], torch.zeros_like(nxt_val)), nxt_val)
        r = rew[t] if rew_den is None else torch.clamp(rew[t] / rew_den, -10.0, 10.0)
        delta = r + gamma * boot - val[t]
        a = delta + gamma * lam * torch.where(d, torch.zeros_like(nxt_adv), nxt_adv)
        adv[t] = a
        if disc is not None:
            disc[t] = rew[t] + gamma * torch.where(d, boot, nxt_ret)
            nxt_ret = disc[t]
        nxt_adv, nxt_val = a, val[t]
    return (adv, adv + val, disc) if with_discounted else (adv, adv + val)


def gae_device(rew, val, done_u8, trunc_u8, last_val, trunc_val, gamma: float = 0.99, lam: float = 0.95,
               rew_den: float | None = None, with_discounted: bool = False, out=None):
    """``gae`` as one HIP launch (cf2_gae): one thread per env scans T backward.  out: optional
    (adv, ret, disc) [T, N] float32 buffers to write."""
    from . import _native
    T, n = rew.shape
    if out is not None:
        adv, ret, disc = out
        for b in (adv, ret) + ((disc,) if with_discounted else ()):
            if b.shape != rew.shape or b.dtype != torch.float32 or not b.is_contiguous() or b.device != rew.device:
                raise ValueError("gae_device out buffers must be contiguous float32 [T, N] on the same device")
        disc = disc if with_discounted else None
    else:
        adv = torch.empty_like(rew)
        ret = torch.empty_like(rew)
        disc = torch.empty_like(rew) if with_discounted else None
    lib = _native.load()
    _native.check(lib.cf2_gae(T, n, rew.contiguous().data_ptr(), val.contiguous().data_ptr(),
                              done_u8.contiguous().data_ptr(), trunc_u8.contiguous().data_ptr(),
                              trunc_val.contiguous().data_ptr(), last_val.contiguous().data_ptr(), float(gamma),
                              float(lam), float(rew_den) if rew_den is not None else 0.0, adv.data_ptr(),
                              ret.data_ptr(), _native.ptr(disc), torch.cuda.current_stream(rew.device).cuda_stream),
                  "cf2_gae")
    return (adv, ret, disc) if with_discounted else (adv, ret)


class EpisodeStats:
    """The epoch log's EpRet / EpLen / EpCosts (iwpg.py:372-410: roll_out stores them at every
    episode end, the logger prints mean, std, min and max) for envs that auto-reset on the device:
    per-env running sums carried from one collect to the next, and a 16-double summary of the
    episodes that finished (cf2_episode_stats, csrc/cf2sim_stats.hip; layout in include/cf2sim.h).
    Pass one to ``collect(..., stats=)`` every epoch and read ``summary()`` once per epoch."""

    KEYS = ("EpRet", "EpLen", "EpCosts")      # at raw()[1:5], [5:9], [9:13]: sum, sumsq, min, max

    def __init__(self, num_envs: int, device):
        from . import _native
        self.lib = _native.load()
        self.num_envs = int(num_envs)
        if self.num_envs <= 0:
            raise ValueError(f"num_envs must be positive, got {num_envs}")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        n, dev = self.num_envs, self.device
        self.ep_ret = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ep_cost = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ep_len = torch.zeros(n, dtype=torch.int32, device=dev)
        self._summary = torch.zeros(16, dtype=torch.float64, device=dev)
        self._scratch = torch.empty(self.lib.cf2_episode_stats_scratch_bytes(n) // 8, dtype=torch.float64, device=dev)
        self._all_costs = True                # every update since the last clear was given costs

    def reset(self, mask: torch.Tensor | None = None) -> None:
        """Forget the running episodes of all envs, or of the masked ones ([N] bool / uint8): call
        it after an ``envs.reset(...)`` that abandons them.  The summary is kept."""
        if mask is None:
            self.ep_ret.zero_(); self.ep_cost.zero_(); self.ep_len.zero_()
            return
        m = torch.as_tensor(mask).to(device=self.device).bool()
        if tuple(m.shape) != (self.num_envs,):
            raise ValueError(f"mask must have shape ({self.num_envs},), got {tuple(m.shape)}")
        self.ep_ret.masked_fill_(m, 0.0); self.ep_cost.masked_fill_(m, 0.0); self.ep_len.masked_fill_(m, 0)

    @torch.no_grad()
    def update(self, rew: torch.Tensor, done: torch.Tensor, cost: torch.Tensor | None = None,
               ep_ret_out: torch.Tensor | None = None, ep_len_out: torch.Tensor | None = None,
               ep_cost_out: torch.Tensor | None = None) -> None:
        """Scan [T, N] (or [N]: one step) rewards, done flags (uint8 or bool) and optional costs
        forward in time and add the episodes that finished to the running summary.  ep_*_out:
        optional [T, N] float32 / int32 / float32 buffers that receive a finished episode's return,
        length and cost in the slot of its last step (other slots are left untouched)."""
        from . import _native
        from .vec_env import _check_buf
        if not isinstance(rew, torch.Tensor) or rew.dim() not in (1, 2):
            raise ValueError("rew must be a [T, N] or [N] torch tensor")
        shape = (1, self.num_envs) if rew.dim() == 1 else (rew.shape[0], self.num_envs)
        flat = rew.dim() == 1
        if isinstance(done, torch.Tensor) and done.dtype == torch.bool:
            done = done.view(torch.uint8)        # same bytes (0 / 1), no copy
        bufs = {"rew": (rew, torch.float32), "done": (done, torch.uint8), "cost": (cost, torch.float32),
                "ep_ret_out": (ep_ret_out, torch.float32), "ep_len_out": (ep_len_out, torch.int32),
                "ep_cost_out": (ep_cost_out, torch.float32)}
        for name, (t, dt) in bufs.items():
            if t is None and name in ("rew", "done"):
                raise ValueError(f"{name} is required")
            _check_buf(t, name, shape[1:] if flat else shape, dt, self.device, align=1 if dt == torch.uint8 else 4)
        if shape[0] == 0:
            return
        _native.check(self.lib.cf2_episode_stats(
            shape[0], shape[1], rew.data_ptr(), _native.ptr(cost), done.data_ptr(), self.ep_ret.data_ptr(),
            self.ep_cost.data_ptr(), self.ep_len.data_ptr(), _native.ptr(ep_ret_out), _native.ptr(ep_len_out),
            _native.ptr(ep_cost_out), self._summary.data_ptr(), 1, self._scratch.data_ptr(),
            torch.cuda.current_stream(self.device).cuda_stream), "cf2_episode_stats")
        self._all_costs = self._all_costs and cost is not None

    def raw(self) -> torch.Tensor:
        """The 16-double device summary (a copy): what ranks gather for ``merge_raw``."""
        return self._summary.clone()

    @staticmethod
    def merge_raw(raws) -> torch.Tensor:
        """Combine summaries (CPU tensors or arrays of 16 doubles, e.g. every rank's ``raw()``):
        counts and sums add, minima and maxima combine, a summary with count 0 is ignored."""
        import numpy as np
        out = np.zeros(16)
        out[[3, 7, 11]], out[[4, 8, 12]] = np.inf, -np.inf
        for r in raws:
            r = np.asarray(r.detach().cpu() if isinstance(r, torch.Tensor) else r, dtype=np.float64).reshape(-1)
            if r.shape != (16,):
                raise ValueError(f"a raw summary has 16 entries, got {r.shape}")
            if not r[0] > 0:
                continue
            out[0] += r[0]
            for k in (1, 5, 9):
                out[k] += r[k]
                out[k + 1] += r[k + 1]
                out[k + 2] = min(out[k + 2], r[k + 2])
                out[k + 3] = max(out[k + 3], r[k + 3])
        return torch.from_numpy(out)

    @staticmethod
    def summary_of(raw, with_costs: bool = True) -> dict:
        """The log entries of a raw summary: ``episodes`` and, per key, mean / std / min / max (the
        population std, as the reference's logger computes it; NaN mean and std with no episode)."""
        import numpy as np
        r = np.asarray(raw.detach().cpu() if isinstance(raw, torch.Tensor) else raw, dtype=np.float64).reshape(-1)
        cnt = r[0] if r[0] > 0 else 0.0
        out = {"episodes": int(cnt)}
        for key, k in zip(EpisodeStats.KEYS, (1, 5, 9)):
            if key == "EpCosts" and not with_costs:
                continue
            if cnt > 0:
                mean = r[k] / cnt
                std = math.sqrt(max(r[k + 1] / cnt - mean * mean, 0.0))
                out[key] = {"mean": mean, "std": std, "min": float(r[k + 2]), "max": float(r[k + 3])}
            else:
                out[key] = {"mean": math.nan, "std": math.nan, "min": math.inf, "max": -math.inf}
        return out

    def summary(self, clear: bool = True) -> dict:
        """Synchronise and return the finished episodes' statistics since the last clear (episodes
        still running are not counted).  ``EpCosts`` is present only if every update since then was
        given costs.  clear=True empties the summary; the per-env carries stay."""
        out = self.summary_of(self._summary.cpu(), with_costs=self._all_costs)
        if clear:
            self._summary.zero_()
            self._all_costs = True
        return out


class LevelOutcomes:
    """Episode outcomes per disturbance level: ``EpisodeStats`` with the finished episodes binned by
    the level they ran under and split into crashes and time-outs (cf2_level_outcomes,
    csrc/cf2sim_outcomes.hip; row layout in include/cf2sim.h) -- the reference's episodic_data.csv
    (episode, disturbance level, steps, return) and per-level evaluation (utils/evaluation.py) for
    envs that auto-reset on the device.  It owns the per-env carries, the [L + 1, 16] table (row L:
    episodes whose level is none of ``level_values``), the scratch and an optional per-env quota.
    Pass one to ``collect(..., outcomes=)`` every epoch, or feed ``update`` yourself, and read
    ``summary()``.  ``set_quota(E)`` makes it count exactly E episodes of every env (``evaluate``)."""

    def __init__(self, num_envs: int, device, level_values):
        import numpy as np
        from . import _native
        self.lib = _native.load()
        self.num_envs = int(num_envs)
        if self.num_envs <= 0:
            raise ValueError(f"num_envs must be positive, got {num_envs}")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        lv = np.asarray(level_values, dtype=np.float64).reshape(-1).astype(np.float32)   # the cast of cf2sim_api.cpp
        if not 1 <= lv.size <= 32:
            raise ValueError(f"between 1 and 32 level values, got {lv.size}")
        self.level_values = lv
        self.num_levels = int(lv.size)
        n, dev = self.num_envs, self.device
        self._levels_dev = torch.from_numpy(lv.copy()).to(dev)
        self.ep_ret = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ep_cost = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ep_len = torch.zeros(n, dtype=torch.int32, device=dev)
        self.episodes_left = None             # [N] int32 once set_quota(E) was called
        self._table = torch.zeros(self.num_levels + 1, 16, dtype=torch.float64, device=dev)
        self._scratch = None
        self._all_costs = True                # every update since the last clear was given costs

    @staticmethod
    def default_level_values(cfg):
        """The levels an env of configuration ``cfg`` can report: ``cfg.level_values[:num_levels]`` for
        Boltzmann-level envs, ``[cfg.dstb_level]`` otherwise."""
        if int(cfg.level_mode) == 1:
            return [float(cfg.level_values[k]) for k in range(int(cfg.num_levels))]
        return [float(cfg.dstb_level)]

    @classmethod
    def for_env(cls, envs) -> "LevelOutcomes":
        return cls(envs.num_envs, envs.device, cls.default_level_values(envs.cfg))

    def reset(self, mask: torch.Tensor | None = None) -> None:
        """Forget the running episodes of all envs, or of the masked ones ([N] bool / uint8): call
        it after an ``envs.reset(...)`` that abandons them.  The table and the quota are kept."""
        if mask is None:
            self.ep_ret.zero_(); self.ep_cost.zero_(); self.ep_len.zero_()
            return
        m = torch.as_tensor(mask).to(device=self.device).bool()
        if tuple(m.shape) != (self.num_envs,):
            raise ValueError(f"mask must have shape ({self.num_envs},), got {tuple(m.shape)}")
        self.ep_ret.masked_fill_(m, 0.0); self.ep_cost.masked_fill_(m, 0.0); self.ep_len.masked_fill_(m, 0)

    def set_quota(self, episodes_per_env: int | None) -> None:
        """Record at most ``episodes_per_env`` further episodes of every env (None: no limit).  With
        auto-resetting envs a crashing env finishes more episodes than a surviving one; a quota keeps
        an evaluation from weighting the short episodes more."""
        if episodes_per_env is None:
            self.episodes_left = None
            return
        if int(episodes_per_env) < 0:
            raise ValueError(f"episodes_per_env must not be negative, got {episodes_per_env}")
        self.episodes_left = torch.full((self.num_envs,), int(episodes_per_env), dtype=torch.int32, device=self.device)

    def remaining(self) -> int:
        """Episodes the quota still waits for, over all envs (one host read; 0 without a quota)."""
        return 0 if self.episodes_left is None else int(self.episodes_left.sum().item())

    @torch.no_grad()
    def update(self, rew: torch.Tensor, done: torch.Tensor, trunc: torch.Tensor | None = None,
               cost: torch.Tensor | None = None, level: torch.Tensor | None = None) -> None:
        """Scan [T, N] (or [N]: one step) rewards, done and truncation flags (uint8 or bool), costs
        and levels forward in time and add the episodes that finished to the table.  Without
        ``trunc`` no crash or time-out is counted, without ``level`` every episode goes to row 0."""
        from . import _native
        from .vec_env import _check_buf
        if not isinstance(rew, torch.Tensor) or rew.dim() not in (1, 2):
            raise ValueError("rew must be a [T, N] or [N] torch tensor")
        shape = (1, self.num_envs) if rew.dim() == 1 else (rew.shape[0], self.num_envs)
        flat = rew.dim() == 1
        if isinstance(done, torch.Tensor) and done.dtype == torch.bool:
            done = done.view(torch.uint8)        # same bytes (0 / 1), no copy
        if isinstance(trunc, torch.Tensor) and trunc.dtype == torch.bool:
            trunc = trunc.view(torch.uint8)
        bufs = {"rew": (rew, torch.float32), "done": (done, torch.uint8), "trunc": (trunc, torch.uint8),
                "cost": (cost, torch.float32), "level": (level, torch.float32)}
        for name, (t, dt) in bufs.items():
            if t is None and name in ("rew", "done"):
                raise ValueError(f"{name} is required")
            _check_buf(t, name, shape[1:] if flat else shape, dt, self.device, align=1 if dt == torch.uint8 else 4)
        if shape[0] == 0:
            return
        need = self.lib.cf2_level_outcomes_scratch_bytes(shape[0], shape[1], self.num_levels)
        if self._scratch is None or self._scratch.numel() * 8 < need:
            self._scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        _native.check(self.lib.cf2_level_outcomes(
            shape[0], shape[1], rew.data_ptr(), _native.ptr(cost), done.data_ptr(), _native.ptr(trunc),
            _native.ptr(level), self._levels_dev.data_ptr(), self.num_levels, self.ep_ret.data_ptr(),
            self.ep_cost.data_ptr(), self.ep_len.data_ptr(), _native.ptr(self.episodes_left), self._table.data_ptr(), 1,
            self._scratch.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), "cf2_level_outcomes")
        self._all_costs = self._all_costs and cost is not None

    def raw(self) -> torch.Tensor:
        """The [L + 1, 16] device table (a copy): what ranks gather for ``merge_raw``."""
        return self._table.clone()

    @staticmethod
    def _empty_row():
        import numpy as np
        row = np.zeros(16)
        row[[3, 7, 11]], row[[4, 8, 12]] = np.inf, -np.inf
        return row

    @staticmethod
    def _merge_row(out, row) -> None:
        """row into out (16 doubles each, in place); a row with count 0 is ignored"""
        if not row[0] > 0:
            return
        for j in (0, 13, 14):
            out[j] += row[j]
        for j in (1, 5, 9):
            out[j] += row[j]
            out[j + 1] += row[j + 1]
            out[j + 2] = min(out[j + 2], row[j + 2])
            out[j + 3] = max(out[j + 3], row[j + 3])

    @staticmethod
    def merge_raw(raws) -> torch.Tensor:
        """Combine tables of one shape (CPU tensors or arrays [L + 1, 16], e.g. every rank's ``raw()``)
        row by row as ``EpisodeStats.merge_raw`` combines summaries: counts and sums add, minima and
        maxima combine, a row with count 0 is ignored."""
        import numpy as np
        out = None
        for r in raws:
            r = np.asarray(r.detach().cpu() if isinstance(r, torch.Tensor) else r, dtype=np.float64)
            if r.ndim != 2 or r.shape[1] != 16 or r.shape[0] < 2:
                raise ValueError(f"a raw table is [L + 1, 16], got {r.shape}")
            if out is None:
                out = np.stack([LevelOutcomes._empty_row() for _ in range(r.shape[0])])
            if r.shape != out.shape:
                raise ValueError(f"tables of different shapes: {r.shape} and {out.shape}")
            for k in range(r.shape[0]):
                LevelOutcomes._merge_row(out[k], r[k])
        if out is None:
            raise ValueError("no table to merge")
        return torch.from_numpy(out)

    @staticmethod
    def _entry(row, with_costs: bool) -> dict:
        e = EpisodeStats.summary_of(row, with_costs=with_costs)
        n = e["episodes"]
        crashes, timeouts = (int(row[13]), int(row[14])) if n else (0, 0)
        out = {"episodes": n, "crashes": crashes, "timeouts": timeouts,
               "crash_rate": crashes / n if n else math.nan}
        out.update({k: v for k, v in e.items() if k != "episodes"})
        return out

    @staticmethod
    def table_of(raw, level_values, with_costs: bool = True) -> dict:
        """The log entries of a raw table: ``{"levels": [...], "other": ..., "total": ...}``, each entry
        ``{"episodes", "crashes", "timeouts", "crash_rate", "EpRet": {mean, std, min, max}, "EpLen",
        "EpCosts"}`` (the population std, NaN mean / std / crash_rate with no episode); the per-level
        ones also carry ``"level"``.  "total" merges every row, "other" included."""
        import numpy as np
        r = np.asarray(raw.detach().cpu() if isinstance(raw, torch.Tensor) else raw, dtype=np.float64)
        lv = np.asarray(level_values, dtype=np.float32).reshape(-1)
        if r.shape != (lv.size + 1, 16):
            raise ValueError(f"a raw table for {lv.size} levels is [{lv.size + 1}, 16], got {r.shape}")
        levels = []
        for k in range(lv.size):
            e = {"level": float(lv[k])}
            e.update(LevelOutcomes._entry(r[k], with_costs))
            levels.append(e)
        total = LevelOutcomes._empty_row()
        for row in r:
            LevelOutcomes._merge_row(total, row)
        return {"levels": levels, "other": LevelOutcomes._entry(r[lv.size], with_costs),
                "total": LevelOutcomes._entry(total, with_costs)}

    def summary(self, clear: bool = True) -> dict:
        """Synchronise and return ``table_of`` the episodes recorded since the last clear (episodes
        still running are not counted).  ``EpCosts`` is present only if every update since then was
        given costs.  clear=True empties the table; the carries and the quota stay."""
        out = self.table_of(self._table.cpu(), self.level_values, with_costs=self._all_costs)
        if clear:
            self._table.zero_()
            self._all_costs = True
        return out


@dataclasses.dataclass
class Rollout:
    obs: torch.Tensor        # [T, N, obs_dim]
    act: torch.Tensor        # [T, N, 4]
    rew: torch.Tensor        # [T, N]
    val: torch.Tensor        # [T, N]
    logp: torch.Tensor       # [T, N]
    done: torch.Tensor       # [T, N] bool
    trunc: torch.Tensor      # [T, N] bool
    adv: torch.Tensor        # [T, N]
    ret: torch.Tensor        # [T, N] value-function targets
    last_obs: torch.Tensor   # [N, obs_dim] observation after the last step
    last_val: torch.Tensor   # [N] V(last_obs)
    trunc_val: torch.Tensor  # [T, N] V(pre-reset obs), used where trunc
    discounted_ret: torch.Tensor  # [T, N] per-episode discounted returns (return statistics)
    # the fused path's buffers, re-used by collect(..., out=this rollout)
    storage: dict | None = dataclasses.field(default=None, repr=False, compare=False)
    # with collect(..., outcomes=): the env-steps' info['cost'] and disturbance levels, [T, N], else
    # None.  Init-only variables kept as plain attributes: code that walks dataclasses.fields() to
    # move or cast a rollout's tensors sees the tensors it always saw.
    cost: dataclasses.InitVar[torch.Tensor | None] = None
    level: dataclasses.InitVar[torch.Tensor | None] = None

    def __post_init__(self, cost, level):
        self.cost, self.level = cost, level


def _fused_storage(steps: int, n: int, d: int, dev) -> dict:
    """The fused collect path's rollout storage: observations [T+1, N, D] (slab 0 = the start
    observation), final observations [T, N, D] (rows written where an episode ended), actions,
    values and log-probabilities [T+1, ...] (slab T: the policy call on the last observation),
    rewards, uint8 done / truncation flags and the GAE outputs."""
    e = lambda *shape, dt=torch.float32: torch.empty(*shape, device=dev, dtype=dt)
    return {"key": (steps, n, d, str(dev)), "obs": e(steps + 1, n, d), "fin": e(steps, n, d),
            "act": e(steps + 1, n, 4), "rew": e(steps, n), "val": e(steps + 1, n), "logp": e(steps + 1, n),
            "d8": e(steps, n, dt=torch.uint8), "tr8": e(steps, n, dt=torch.uint8), "trunc_val": e(steps, n),
            "adv": e(steps, n), "ret": e(steps, n), "disc": e(steps, n)}


@torch.no_grad()
def collect(envs, ac, steps: int, obs: torch.Tensor | None = None, gamma: float = 0.99,
            lam: float = 0.95, generator: torch.Generator | None = None, fuse: bool | str = True,
            out: Rollout | None = None, stats: EpisodeStats | None = None,
            outcomes: "LevelOutcomes | None" = None) -> Rollout:
    """``roll_out`` for all envs of a BatchedCrazyflieEnv at once; everything stays on the GPU.
    ``ac`` is an MLPActorCritic (torch layers) or a FusedActorCritic (HIP kernels).  With a
    FusedActorCritic, ``fuse`` picks how the loop's env-steps and policy calls are launched where
    the config has fused instances: True -- all ``steps`` of them in one launch
    (cf2_collect_rollout, the env state in registers throughout); "steps" -- one launch per
    env-step (cf2_collect_step); False -- two launches per env-step.  The results are
    bit-identical in every mode, and a config without fused instances runs the two launches.
    ``out``: a Rollout of an earlier fused collect of the
    same shape whose storage is re-used (its tensors are overwritten; ``obs=out.last_obs`` is
    allowed), as a training loop collecting every epoch would.
    ``stats``: an EpisodeStats that follows the envs' episodes through this collect (reset with
    the envs when ``obs`` is None, then updated from the rollout's rewards and done flags; the
    torch-module path also hands it the per-step costs, and so does the fused path when
    ``outcomes`` is given).
    ``outcomes``: a LevelOutcomes that follows the episodes likewise, per disturbance level.  Only
    then do the env-steps also write their cost and level ([T, N], ``Rollout.cost`` / ``.level``; on
    the fused path slabs of the storage, through cf2_collect_step_info / cf2_collect_rollout_info);
    every other output is what it is without it, bit for bit.
    ``envs`` must have been created with want_final_obs=True (time-out bootstrapping)."""
    if envs.final_obs is None:
        raise ValueError("collect() needs BatchedCrazyflieEnv(..., want_final_obs=True)")
    n, d, dev = envs.num_envs, envs.obs_dim, envs.device
    o = envs.reset() if obs is None else obs
    if stats is not None and obs is None:
        stats.reset()
    if outcomes is not None and obs is None:
        outcomes.reset()
    fused = isinstance(ac, FusedActorCritic)
    module = ac.ac if fused else ac
    rew_den = module.ret_oms.std_host() + module.ret_oms.eps if module.ret_oms is not None else None
    if fused:
        # zero-copy: the policy and the env write straight into the rollout storage
        S = out.storage if out is not None and out.storage is not None else None
        if S is None or S["key"] != (steps, n, d, str(dev)):
            S = _fused_storage(steps, n, d, dev)
        obs_buf, fin, act_all, buf_r, val_all, lp_all = S["obs"], S["fin"], S["act"], S["rew"], S["val"], S["logp"]
        buf_a, buf_v, buf_lp, last_val = act_all[:steps], val_all[:steps], lp_all[:steps], val_all[steps]
        d8, tr8, trunc_val = S["d8"], S["tr8"], S["trunc_val"]
        buf_c = buf_l = None
        info_kw = {}
        if outcomes is not None:
            if "cost" not in S:
                S["cost"], S["level"] = torch.empty(steps, n, device=dev), torch.empty(steps, n, device=dev)
            buf_c, buf_l = S["cost"], S["level"]
            info_kw = {"cost_out": buf_c, "level_out": buf_l}
        obs_buf[0].copy_(o)
        trunc_val.zero_()                 # read only where truncated; zero elsewhere, as the torch path
        # the policy of step t + 1 runs right behind the env-step of step t (fused: in its launch);
        # the last one gives V(obs_T), its sampled action and logp are not used
        roff = int(envs.cfg.env_id_offset)    # sampling noise keyed by the global env id
        ac.step_into(obs_buf[0], act_all[0], val_all[0], lp_all[0], row_offset=roff)
        if fuse is True and not envs.collect_rollout_into(act_all, obs_buf[1:], buf_r, d8, tr8, fin, ac, val_all,
                                                          lp_all, **info_kw):
            fuse = False                       # no fused instance for this config: two launches per step
        for t in range(steps if fuse is True else 0, steps):
            nxt = (act_all[t + 1], val_all[t + 1], lp_all[t + 1])
            if fuse and t == 0:
                # the first step goes through every buffer check; the later slabs have the same
                # shapes, so the loop then passes raw pointers (slab strides) to keep ahead of the GPU
                if envs.collect_step_into(buf_a[0], obs_buf[1], buf_r[0], d8[0], tr8[0], fin[0], ac, *nxt,
                                          **{k: v[0] for k, v in info_kw.items()}):
                    continue
                fuse = False
            elif fuse:
                sa, so, sf = n * 16, n * d * 4, n * 4            # slab strides in bytes
                a_p, o_p, r_p, v_p, l_p, f_p = (buf_a.data_ptr(), obs_buf.data_ptr(), buf_r.data_ptr(),
                                                buf_v.data_ptr(), buf_lp.data_ptr(), fin.data_ptr())
                dp, tp = d8.data_ptr(), tr8.data_ptr()
                c_p, lv_p = (buf_c.data_ptr(), buf_l.data_ptr()) if outcomes is not None else (None, None)
                for u in range(t, steps):
                    nx = (a_p + (u + 1) * sa, v_p + (u + 1) * sf, l_p + (u + 1) * sf)
                    if outcomes is not None:
                        nx += (c_p + u * sf, lv_p + u * sf)
                    if not envs.collect_step_raw(a_p + u * sa, o_p + (u + 1) * so, r_p + u * sf, dp + u * n, tp + u * n,
                                                 f_p + u * so, ac, *nx):
                        raise RuntimeError("cf2_collect_step stopped being supported inside a collect")
                envs._obs_latest = obs_buf[steps]    # what save_checkpoint saves after this collect
                break
            envs.step_into(buf_a[t], obs_buf[t + 1], buf_r[t], d8[t], tr8[t], final_obs_out=fin[t],
                           **{k: v[t] for k, v in info_kw.items()})
            ac.step_into(obs_buf[t + 1], *nxt, row_offset=roff)
        per = max(1, (2**31 - 1) // n)                      # row counts of the C ABI are 32-bit
        for t0 in range(0, steps, per):                      # V(final obs) of the time-outs only
            t1 = min(steps, t0 + per)
            ac.value_masked(fin[t0:t1].view(-1, d), tr8[t0:t1].view(-1), trunc_val[t0:t1].view(-1))
        envs.last_collect_fused = fuse         # True / "steps": every env-step ran fused (the mode that ran)
        o = obs_buf[steps]
        adv, ret, disc = gae_device(buf_r, buf_v, d8, tr8, last_val, trunc_val, gamma, lam, rew_den, True,
                                    out=(S["adv"], S["ret"], S["disc"]))
        buf_o, buf_d, buf_tr = obs_buf[:steps], d8.view(torch.bool), tr8.view(torch.bool)   # 0/1 bytes
        if stats is not None:
            stats.update(buf_r, d8, buf_c)    # costs only with outcomes=: cf2_collect_step writes none
        if outcomes is not None:
            outcomes.update(buf_r, d8, tr8, buf_c, buf_l)
        return Rollout(buf_o, buf_a, buf_r, buf_v, buf_lp, buf_d, buf_tr, adv, ret, o, last_val, trunc_val, disc,
                       storage=S, cost=buf_c, level=buf_l)
    buf_o = torch.empty(steps, n, d, device=dev)
    buf_a = torch.empty(steps, n, 4, device=dev)
    buf_r = torch.empty(steps, n, device=dev)
    buf_v = torch.empty(steps, n, device=dev)
    buf_lp = torch.empty(steps, n, device=dev)
    buf_d = torch.empty(steps, n, dtype=torch.bool, device=dev)
    buf_tr = torch.empty(steps, n, dtype=torch.bool, device=dev)
    trunc_val = torch.zeros(steps, n, device=dev)
    buf_c = torch.empty(steps, n, device=dev) if stats is not None or outcomes is not None else None
    buf_l = torch.empty(steps, n, device=dev) if outcomes is not None else None
    for t in range(steps):
        a, v, lp = ac.step(o, generator=generator)
        buf_o[t] = o
        buf_a[t] = a
        buf_v[t] = v
        buf_lp[t] = lp
        o, r, dn, info = envs.step(a.contiguous())
        buf_r[t] = r
        buf_d[t] = dn.bool()
        buf_tr[t] = info["truncated"].bool()
        if buf_c is not None:
            buf_c[t] = info["cost"]
        if buf_l is not None:
            buf_l[t] = info["disturbance_level"]
        trunc_val[t] = ac.value(info["final_obs"])      # only read where truncated
    last_val = ac.value(o)
    adv, ret, disc = gae(buf_r, buf_v, buf_d, buf_tr, last_val, trunc_val, gamma, lam, rew_den, True)
    if stats is not None:
        stats.update(buf_r, buf_d, buf_c)
    if outcomes is not None:
        outcomes.update(buf_r, buf_d, buf_tr, buf_c, buf_l)
    return Rollout(buf_o, buf_a, buf_r, buf_v, buf_lp, buf_d, buf_tr, adv, ret, o, last_val, trunc_val, disc,
                   cost=buf_c if outcomes is not None else None, level=buf_l)


__all__ = ["OnlineMeanStd", "MLPActorCritic", "FusedActorCritic", "pack_policy_weights", "unpack_policy_weights", "gae", "gae_device", "collect",
           "Rollout", "update_running_statistics", "EpisodeStats", "LevelOutcomes"]
