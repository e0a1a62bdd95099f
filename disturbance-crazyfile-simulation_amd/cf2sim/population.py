"""Populations: P independent learners (seeds, hyper-parameter settings) on one BatchedCrazyflieEnv.

One learner trains on 4 096 - 32 768 envs, where every launch is a latency chain; P learners run one
after the other pay it P times.  The env side of a population is free: every draw of the env kernels
is keyed by the global env id, so one context of P * n envs is bit for bit P contexts of n envs with
``env_id_offset = m * n``.  This module is the policy side:

* ``Population``: P ``MLPActorCritic`` modules, one ``[P, stride]`` block of packed weights and the
  device array of the P noise seeds; ``step_into`` is one launch over all P * n rows
  (cf2_policy_forward_pop, csrc/cf2sim_population.hip), member m's rows through member m's weights
  with the noise of (seed_m, call counter, global row).  ``member(m)`` is a ``FusedActorCritic``
  whose packed block is member m's slice of the population's, for everything that runs per member:
  ``value_masked``, ``update_running_statistics`` and the updaters' ``fused=``.
* ``collect_population``: ``collect``'s two-launch loop for all members at once, one move of the
  storage into member-major buffers ``[P, T, n, ...]`` (torch plumbing), then the single-learner
  code per member on its contiguous slice: time-out values, GAE with the member's own return
  statistics, the member's ``EpisodeStats``.

Every member's whole training run is bit-identical to the run it has alone on
``BatchedCrazyflieEnv(id, n, seed=s, env_id_offset=m * n)`` with ``FusedActorCritic(ac_m, seed_m)``
(tests/test_population_gpu.py).  Not covered: per-member weights inside the fused collect kernels,
one-launch gradients for all members (updates run member after member), ``group=`` and formations.
"""
from __future__ import annotations

import dataclasses

import torch

from .rollout import (POLICY_PRECISIONS, EpisodeStats, FusedActorCritic, MLPActorCritic, Rollout, gae_device,
                      pack_policy_weights)


def rows_per_member(num_rows: int, members: int) -> int:
    """n of ``num_rows = members * n``; ValueError where the rows do not split evenly."""
    num_rows, members = int(num_rows), int(members)
    if members <= 0:
        raise ValueError(f"a population has at least one member, got {members}")
    if num_rows <= 0 or num_rows % members != 0:
        raise ValueError(f"{num_rows} rows do not split into {members} members of equal size")
    return num_rows // members


def member_major(x: torch.Tensor, members: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """``[T, P * n, ...]`` -> contiguous ``[P, T, n, ...]``: ``out[m] == x[:, m * n:(m + 1) * n]``, one
    strided copy (``out``: a buffer of that shape and dtype to fill)."""
    if x.dim() < 2:
        raise ValueError(f"expected [T, N, ...], got {tuple(x.shape)}")
    T, n = x.shape[0], rows_per_member(x.shape[1], members)
    shape = (members, T, n, *x.shape[2:])
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {x.dtype} tensor of shape {shape} on {x.device}")
    out.copy_(x.reshape(T, members, n, *x.shape[2:]).transpose(0, 1))
    return out


class PopulationMember(FusedActorCritic):
    """``Population.member(m)``: a FusedActorCritic over member m's module whose packed block ``w`` is
    the member's slice of the population's block -- ``sync`` / ``sync_from_flat`` pack into it in
    place -- and whose call counter is the population's."""

    def __init__(self, pop: "Population", m: int):
        self.pop, self.index = pop, m
        self.ac = pop.acs[m]
        self.lib = pop.lib
        self.seed = pop.seeds[m]
        self.precision, self.prec, self.obs_dim = pop.precision, pop.prec, pop.obs_dim
        self.w = pop.w[m, :pop.packed_count]
        self.w_ptr = self.w.data_ptr()

    @property
    def counter(self) -> int:
        return self.pop.counter

    @counter.setter
    def counter(self, value: int) -> None:
        self.pop.counter = int(value)

    def sync_from_flat(self, flat: torch.Tensor):
        from . import _native
        dev = self.w.device
        count = self.lib.cf2_policy_weights_count(self.obs_dim)
        if not isinstance(flat, torch.Tensor) or flat.dtype != torch.float32 or flat.device != dev \
                or not flat.is_contiguous() or flat.numel() != count:
            raise ValueError(f"flat must be a contiguous float32 block of {count} words on {dev}")
        _native.check(self.lib.cf2_policy_pack(flat.data_ptr(), self.obs_dim, self.prec, self.w_ptr,
                                               torch.cuda.current_stream(dev).cuda_stream), "cf2_policy_pack")


class Population:
    """P independent learners whose policy forward is one launch.  ``acs``: P MLPActorCritic modules of
    one observation size on one GPU; ``seeds``: their P noise seeds (what each would give its own
    ``FusedActorCritic``).  Call ``sync()`` (or a member's) after changing a module's parameters."""

    def __init__(self, acs, seeds, precision: str = "bf16x3"):
        acs, seeds = list(acs), [int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]
        if not acs:
            raise ValueError("a population has at least one member")
        if len(seeds) != len(acs):
            raise ValueError(f"{len(acs)} members need {len(acs)} seeds, got {len(seeds)}")
        if precision not in POLICY_PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(POLICY_PRECISIONS)}, got {precision!r}")
        if not all(isinstance(ac, MLPActorCritic) for ac in acs):
            raise ValueError("every member must be an MLPActorCritic")
        if len({id(ac) for ac in acs}) != len(acs):
            raise ValueError("every member needs a module of its own")
        dims = {ac.pi_net[0].in_features for ac in acs}
        devs = {next(ac.parameters()).device for ac in acs}
        if len(dims) != 1 or len(devs) != 1:
            raise ValueError(f"the members must share one observation size and one device, got {dims} on {devs}")
        from . import _native
        self.lib = _native.load()
        self.acs, self.seeds = acs, seeds
        self.precision, self.prec = precision, POLICY_PRECISIONS[precision]
        self.obs_dim, self.device = dims.pop(), devs.pop()
        self.counter = 0
        self.packed_count = int(self.lib.cf2_policy_packed_count(self.obs_dim, self.prec))
        if self.packed_count == 0:
            raise ValueError(f"the fused kernel has no instance for obs_dim {self.obs_dim}")
        self.stride = (self.packed_count + 3) // 4 * 4          # every member's block 16-B aligned
        self.w = torch.empty(len(acs), self.stride, device=self.device)
        # int64 carries the uint64 bit pattern (the kernel reads the words as unsigned)
        self.seeds_dev = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64,
                                      device=self.device)
        self._members = [PopulationMember(self, m) for m in range(len(acs))]
        self.sync()

    def __len__(self) -> int:
        return len(self.acs)

    def member(self, m: int) -> PopulationMember:
        return self._members[m]

    def sync(self) -> None:
        """Re-pack every member's weights into the population block."""
        for v in self._members:
            v.sync_from_flat(pack_policy_weights(v.ac).to(self.device))

    @torch.no_grad()
    def step_into(self, obs: torch.Tensor, act: torch.Tensor, val: torch.Tensor, logp: torch.Tensor | None,
                  row_offset: int = 0, deterministic: bool = False) -> None:
        """``FusedActorCritic.step_into`` for all members in one launch: obs ``[P * n, D]``, member m
        owning rows ``[m * n, (m + 1) * n)``; the noise of row r is keyed (seed of r's member, call
        counter, row_offset + r).  Advances the call counter every member shares."""
        from . import _native
        from .vec_env import _check_buf
        N = int(obs.shape[0]) if isinstance(obs, torch.Tensor) and obs.dim() == 2 else 0
        n = rows_per_member(N, len(self))
        _check_buf(obs, "obs", (N, self.obs_dim), torch.float32, self.device, 8)
        _check_buf(act, "act", (N, 4), torch.float32, self.device, 16)
        _check_buf(val, "val", (N,), torch.float32, self.device)
        _check_buf(logp, "logp", (N,), torch.float32, self.device)
        if act is None or val is None:
            raise ValueError("act and val are required")
        _native.check(self.lib.cf2_policy_forward_pop(
            self.w.data_ptr(), self.stride, len(self), n, self.obs_dim, self.prec, obs.data_ptr(),
            self.seeds_dev.data_ptr(), self.counter & 0xFFFFFFFF, int(row_offset) & 0xFFFFFFFF,
            0 if deterministic else 1, act.data_ptr(), val.data_ptr(), _native.ptr(logp),
            torch.cuda.current_stream(self.device).cuda_stream), "cf2_policy_forward_pop")
        self.counter += 1


@dataclasses.dataclass
class PopulationRollout:
    members: list            # P Rollouts [T, n, ...], contiguous slices of the member-major storage
    last_obs: torch.Tensor   # [P * n, obs_dim] observation after the last step: obs= of the next collect
    storage: dict = dataclasses.field(default=None, repr=False, compare=False)


# the collect loop's [T(+1), N, ...] buffers that move into member-major storage: (name, slabs beyond T)
_MOVED = (("obs", 1), ("fin", 0), ("act", 0), ("rew", 0), ("val", 1), ("logp", 0), ("d8", 0), ("tr8", 0))


def _loop_storage(steps: int, N: int, d: int, dev) -> dict:
    e = lambda *shape, dt=torch.float32: torch.empty(*shape, device=dev, dtype=dt)
    return {"obs": e(steps + 1, N, d), "fin": e(steps, N, d), "act": e(steps + 1, N, 4), "rew": e(steps, N),
            "val": e(steps + 1, N), "logp": e(steps + 1, N), "d8": e(steps, N, dt=torch.uint8),
            "tr8": e(steps, N, dt=torch.uint8)}


def _member_storage(steps: int, P: int, n: int, d: int, dev) -> dict:
    e = lambda *shape, dt=torch.float32: torch.empty(*shape, device=dev, dtype=dt)
    return {"obs": e(P, steps + 1, n, d), "fin": e(P, steps, n, d), "act": e(P, steps, n, 4), "rew": e(P, steps, n),
            "val": e(P, steps + 1, n), "logp": e(P, steps, n), "d8": e(P, steps, n, dt=torch.uint8),
            "tr8": e(P, steps, n, dt=torch.uint8), "trunc_val": e(P, steps, n), "adv": e(P, steps, n),
            "ret": e(P, steps, n), "disc": e(P, steps, n)}


@torch.no_grad()
def collect_population(envs, pop: Population, steps: int, obs: torch.Tensor | None = None, gamma: float = 0.99,
                       lam: float = 0.95, out: PopulationRollout | None = None, stats=None) -> PopulationRollout:
    """``collect`` for the P members of ``pop`` on one BatchedCrazyflieEnv of exactly P * n envs (created
    with want_final_obs=True), member m flying envs ``[m * n, (m + 1) * n)``.  Two launches per
    env-step for the whole population (``envs.step_into``, ``pop.step_into``), one move of the
    rollout storage into member-major buffers, then per member the time-out values
    (``value_masked``), ``gae_device`` with the member's own return statistics and, with ``stats``
    (a list of P EpisodeStats, each for n envs), the member's episode log.
    ``members[m]`` of the result is the Rollout member m collects alone, bit for bit; pass
    ``obs=result.last_obs`` and ``out=result`` to continue into the same storage."""
    if envs.final_obs is None:
        raise ValueError("collect_population() needs BatchedCrazyflieEnv(..., want_final_obs=True)")
    P = len(pop)
    N = int(envs.num_envs)
    n = rows_per_member(N, P)
    steps = int(steps)
    if steps <= 0:
        raise ValueError(f"steps must be positive, got {steps}")
    d, dev = envs.obs_dim, envs.device
    if d != pop.obs_dim or torch.device(dev) != pop.device:
        raise ValueError(f"the population runs {pop.obs_dim}-dim observations on {pop.device}, the envs {d} on {dev}")
    if stats is not None:
        stats = list(stats)
        if len(stats) != P or any(not isinstance(s, EpisodeStats) or s.num_envs != n for s in stats):
            raise ValueError(f"stats must be {P} EpisodeStats of {n} envs each")
    o = envs.reset() if obs is None else obs
    if stats is not None and obs is None:
        for s in stats:
            s.reset()
    key = (steps, P, n, d, str(dev))
    S = out.storage if out is not None and out.storage is not None and out.storage["key"] == key else None
    if S is None:
        S = {"key": key, "loop": _loop_storage(steps, N, d, dev), "member": _member_storage(steps, P, n, d, dev)}
    L, M = S["loop"], S["member"]
    obs_buf, fin, act_all, val_all, lp_all = L["obs"], L["fin"], L["act"], L["val"], L["logp"]
    obs_buf[0].copy_(o)
    roff = int(envs.cfg.env_id_offset)        # sampling noise keyed by the global env id
    pop.step_into(obs_buf[0], act_all[0], val_all[0], lp_all[0], row_offset=roff)
    for t in range(steps):
        envs.step_into(act_all[t], obs_buf[t + 1], L["rew"][t], L["d8"][t], L["tr8"][t], final_obs_out=fin[t])
        pop.step_into(obs_buf[t + 1], act_all[t + 1], val_all[t + 1], lp_all[t + 1], row_offset=roff)
    envs.last_collect_fused = False
    for name, extra in _MOVED:
        member_major(L[name][:steps + extra], P, out=M[name])
    M["trunc_val"].zero_()                    # read only where truncated; zero elsewhere, as collect()
    per = max(1, (2**31 - 1) // n)            # row counts of the C ABI are 32-bit
    rollouts = []
    for m in range(P):
        view, module = pop.member(m), pop.acs[m]
        m_fin, m_tr8, m_tv = M["fin"][m], M["tr8"][m], M["trunc_val"][m]
        for t0 in range(0, steps, per):       # V(final obs) of the member's time-outs only
            t1 = min(steps, t0 + per)
            view.value_masked(m_fin[t0:t1].view(-1, d), m_tr8[t0:t1].view(-1), m_tv[t0:t1].view(-1))
        rew_den = module.ret_oms.std_host() + module.ret_oms.eps if module.ret_oms is not None else None
        m_val, m_rew, m_d8 = M["val"][m], M["rew"][m], M["d8"][m]
        adv, ret, disc = gae_device(m_rew, m_val[:steps], m_d8, m_tr8, m_val[steps], m_tv, gamma, lam, rew_den, True,
                                    out=(M["adv"][m], M["ret"][m], M["disc"][m]))
        if stats is not None:
            stats[m].update(m_rew, m_d8, None)
        rollouts.append(Rollout(M["obs"][m, :steps], M["act"][m], m_rew, m_val[:steps], M["logp"][m],
                                m_d8.view(torch.bool), m_tr8.view(torch.bool), adv, ret, M["obs"][m, steps],
                                m_val[steps], m_tv, disc))
    return PopulationRollout(rollouts, obs_buf[steps], storage=S)


__all__ = ["Population", "PopulationMember", "PopulationRollout", "collect_population", "member_major",
           "rows_per_member"]
