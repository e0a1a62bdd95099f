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
* ``PopulationPPOUpdater``: the resident PPO update of all members as one launch sequence whose
  length does not depend on P (cf2_ppo_policy_grad_pop, cf2_ppo_value_grad_pop, cf2_adam_step_pop),
  reading the member-major storage in place; per-member learning rates, clip ratios, KL targets and
  gradient-norm limits, each member stopping at its own iteration.
* ``PopulationNaturalGradientUpdater``: the resident TRPO / NPG update of all members likewise
  (cf2_ppo_fisher_vec_pop and the four cf2_ng_*_pop solver launches); per-member KL targets, CG
  dampings, value learning rates and gradient-norm limits, each member's conjugate gradients and
  line search stopping on their own.

Every member's whole training run is bit-identical to the run it has alone on
``BatchedCrazyflieEnv(id, n, seed=s, env_id_offset=m * n)`` with ``FusedActorCritic(ac_m, seed_m)``
and ``ResidentPPOUpdater(ac_m, ...)`` or ``NaturalGradientUpdater(ac_m, ...)``
(tests/test_population_gpu.py, tests/test_population_update_gpu.py,
tests/test_population_natgrad_gpu.py).  Not covered: per-member weights inside the fused collect
kernels, ``group=`` and formations.
"""
from __future__ import annotations

import dataclasses
import math

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


def per_member(value, members: int, name: str, none=None) -> list:
    """A hyper-parameter of a population as a list of ``members`` floats: a scalar counts for every
    member, a sequence must have one entry per member (ValueError otherwise).  ``none``: the value a
    None (the whole argument or an entry) stands for."""
    if value is None or not hasattr(value, "__len__"):
        value = [value] * members
    value = list(value)
    if len(value) != members:
        raise ValueError(f"{name} must be a scalar or a sequence of {members} values, got {len(value)}")
    if none is None and any(v is None for v in value):
        raise ValueError(f"{name} is required for every member")
    return [float(none if v is None else v) for v in value]


def member_stride(tensors, name: str) -> int:
    """The member stride, in elements, of P equally shaped row buffers that are equally spaced,
    contiguous, non-overlapping slices of one allocation (what ``collect_population`` hands out):
    member k's buffer starts ``k * stride`` elements after member 0's.  ValueError otherwise: the
    population kernels take one base pointer and one stride per buffer, and nothing is copied."""
    tensors = list(tensors)
    t0 = tensors[0]
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.shape != t0.shape or t.dtype != t0.dtype or t.device != t0.device \
                or not t.is_contiguous():
            raise ValueError(f"the members' {name} must be contiguous tensors of one shape, dtype and device")
    if len(tensors) == 1:
        return t0.numel()
    es, base = t0.element_size(), t0.data_ptr()
    step = tensors[1].data_ptr() - base
    if step % es or step < t0.numel() * es or any(t.data_ptr() != base + k * step for k, t in enumerate(tensors)):
        raise ValueError(f"the members' {name} are not equally spaced slices of one buffer: a population updater "
                         "updates from the member-major storage of collect_population")
    return step // es


class _PopulationUpdaterShared:
    """What the population updaters share (``PopulationPPOUpdater``, ``PopulationNaturalGradientUpdater``):
    the per-member optimiser states ``self.opt`` and their ``state_dict``, the view of a
    ``PopulationRollout`` as one base tensor and one member stride per row buffer, the per-member
    plumbing at both ends of an update and the value phase.  A class using it has ``pop``,
    ``generators``, ``count``, ``pi_slice``, ``v_slice``, ``flat``, ``grad``, ``opt``, ``betas``, ``eps``,
    ``v_lr_dev`` (``pi_lr_dev`` where it steps the policy with Adam), ``target_kl_dev``,
    ``max_grad_norm_dev``, ``summary_mb``, ``train_v_iterations`` and ``num_mini_batches``."""

    @staticmethod
    def _check_generators(generators, P: int):
        if generators is not None:
            generators = list(generators)
            if len(generators) != P or any(not isinstance(g, torch.Generator) for g in generators):
                raise ValueError(f"generators must be None or {P} torch.Generators, one per member")
        return generators

    def state_dict(self) -> list:
        return [{w: {"exp_avg": s["exp_avg"][k].clone(), "exp_avg_sq": s["exp_avg_sq"][k].clone(),
                     "step": s["step"][k:k + 1].clone()} for w, s in self.opt.items()} for k in range(len(self.pop))]

    def load_state_dict(self, sd) -> None:
        sd = list(sd)
        if len(sd) != len(self.pop):
            raise ValueError(f"expected {len(self.pop)} entries, one per member, got {len(sd)}")
        for k, entry in enumerate(sd):
            for w, s in self.opt.items():
                s["exp_avg"][k].copy_(entry[w]["exp_avg"])
                s["exp_avg_sq"][k].copy_(entry[w]["exp_avg_sq"])
                s["step"][k:k + 1].copy_(entry[w]["step"])

    def _adam(self, which: str, kl_summary=None, ctrl=None) -> None:
        from . import _native
        s, (b0, b1) = self.opt[which], self.pi_slice if which == "pi" else self.v_slice
        p = _native.ptr
        _native.check(self.pop.lib.cf2_adam_step_pop(
            len(self.pop), p(self.flat), p(self.grad), p(s["exp_avg"]), p(s["exp_avg_sq"]), self.count, b0, b1 - b0,
            p(s["step"]), p(self.pi_lr_dev if which == "pi" else self.v_lr_dev), self.betas[0], self.betas[1], self.eps,
            p(self.max_grad_norm_dev), p(s["norm"]), p(kl_summary), p(self.target_kl_dev), p(ctrl),
            torch.cuda.current_stream(self.flat.device).cuda_stream), "cf2_adam_step_pop")

    def _member_views(self, rollout: "PopulationRollout"):
        """(members, rows, base, stride): the rollout's row buffers as member 0's tensor and the member
        stride in elements, per name; ValueError where they are not the member-major storage."""
        P, d, dev = len(self.pop), self.pop.obs_dim, self.flat.device
        ms = list(rollout.members)
        if len(ms) != P:
            raise ValueError(f"the rollout has {len(ms)} members, the population {P}")
        obs0 = ms[0].obs
        if obs0.dim() != 3 or obs0.shape[-1] != d or obs0.device != dev or obs0.dtype != torch.float32:
            raise ValueError(f"a member's obs must be float32 [T, n, {d}] on {dev}, got {tuple(obs0.shape)} on {obs0.device}")
        rows = obs0.shape[0] * obs0.shape[1]
        if rows == 0 or rows >= 2 ** 31:
            raise ValueError(f"a rollout of {rows} rows per member cannot be updated from in one call")
        want = {"obs": (*obs0.shape[:2], d), "act": (*obs0.shape[:2], 4), "logp": tuple(obs0.shape[:2]),
                "adv": tuple(obs0.shape[:2]), "ret": tuple(obs0.shape[:2])}
        base, stride = {}, {}
        for name, shape in want.items():
            ts = [getattr(r, name) for r in ms]
            if tuple(ts[0].shape) != shape or ts[0].dtype != torch.float32 or ts[0].device != dev:
                raise ValueError(f"a member's {name} must be float32 {shape} on {dev}")
            base[name], stride[name] = ts[0], member_stride(ts, name)
        if stride["obs"] % 2 or stride["act"] % 4 or base["obs"].data_ptr() % 8 or base["act"].data_ptr() % 16:
            raise ValueError("the members' obs must be 8-byte and their act 16-byte aligned")
        return ms, rows, base, stride

    def _begin(self, ms, rows: int, idx, mom, scratch, stream) -> None:
        """Every value pass's permutations, the members' advantage moments and packed flat blocks."""
        from . import _native
        P, dev = len(self.pop), self.flat.device
        # Every value pass's permutations, member k's drawn with generators[k] in pass order exactly as
        # PPOUpdater.value_minibatches draws them, but all before the first launch: torch.randperm on the
        # GPU waits for the work already enqueued (measured at 32 768 and 131 072 rows, not at 1 048 576),
        # which between the passes would stall the host once per member and pass.
        for v in range(self.train_v_iterations):
            for k in range(P):
                g = self.generators[k] if self.generators is not None else None
                idx[v, k].copy_(torch.randperm(rows, generator=g, device=g.device if g is not None else dev))
        for k in range(P):        # per-member plumbing, once per update
            _native.check(self.pop.lib.cf2_column_moments(ms[k].adv.data_ptr(), rows, 1, mom[k].data_ptr(),
                                                          scratch.data_ptr(), stream), "cf2_column_moments")
            self.flat[k].copy_(pack_policy_weights(self.pop.acs[k]))

    def _value_call(self, rows: int, base, stride, scratch, stream):
        """``val(summary, grad=None, idx_ptr=None, m=rows)``: cf2_ppo_value_grad_pop on the rollout."""
        from . import _native
        pop, p = self.pop, _native.ptr

        def val(summ, grad=None, idx_ptr=None, m=rows):
            _native.check(pop.lib.cf2_ppo_value_grad_pop(
                len(pop), p(self.flat), self.count, pop.obs_dim, p(base["obs"]), stride["obs"], p(base["ret"]),
                stride["ret"], rows, idx_ptr, rows, m, None, 0, p(grad), p(summ), p(scratch), None, stream),
                "cf2_ppo_value_grad_pop")
        return val

    def _value_phase(self, val, idx, rows: int) -> None:
        nb = min(self.num_mini_batches, rows)
        for v in range(self.train_v_iterations):
            for j in range(nb):           # the members' j-th pieces of pass v's permutations
                lo, hi = (j * rows) // nb, ((j + 1) * rows) // nb
                val(self.summary_mb, grad=self.grad, idx_ptr=idx[v].data_ptr() + 4 * lo, m=hi - lo)
                self._adam("v")

    def _end(self) -> None:
        from .rollout import unpack_policy_weights
        for k in range(len(self.pop)):
            unpack_policy_weights(self.pop.acs[k], self.flat[k])
            self.pop.member(k).sync_from_flat(self.flat[k])


class PopulationPPOUpdater(_PopulationUpdaterShared):
    """``ResidentPPOUpdater`` for all members of a ``Population`` at once: the launch sequence of one
    resident update, every launch serving the P members (cf2_ppo_policy_grad_pop,
    cf2_ppo_value_grad_pop, cf2_adam_step_pop), so an update is a number of launches that does not
    depend on P.  Member k's update is bit for bit the one
    ``ResidentPPOUpdater(pop.acs[k], pi_lr[k], ..., fused=pop.member(k), generator=generators[k])``
    makes on ``rollout.members[k]`` (tests/test_population_update_gpu.py).

    ``pi_lr``, ``v_lr``, ``clip_ratio``, ``target_kl`` and ``max_grad_norm`` are each a scalar or a
    sequence of P values (members are hyper-parameter settings); the iteration counts, the number of
    mini-batches, the betas and eps are shared.  Every launch of the policy phase is gated per member
    by the member's own control block, so the members stop at their own iterations.  ``generators``:
    None or P torch.Generators, member k's being the one it would give its own updater (the value
    passes' permutations are drawn per member, exactly as ``PPOUpdater.value_minibatches`` draws them,
    all of an update's at its start).

    The row buffers are the rollout's member-major storage, read in place through one base pointer
    and one member stride per buffer.  ``update(rollout, read=False)`` never waits for the GPU;
    ``result()`` reads the P x 6 results in one transfer.  ``state_dict()`` is a list of P entries,
    entry k interchangeable with ``ResidentPPOUpdater.state_dict()`` of the stand-alone learner.
    Per update and member there is still torch plumbing: packing and unpacking the flat block, the
    advantage moments and ``sync_from_flat``."""

    def __init__(self, pop: Population, pi_lr, v_lr, clip_ratio, target_kl, train_pi_iterations: int = 80,
                 train_v_iterations: int = 5, num_mini_batches: int = 16, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm=None, generators=None):
        from .ppo import flat_slice
        P = len(pop)
        self.pi_lr, self.v_lr = per_member(pi_lr, P, "pi_lr"), per_member(v_lr, P, "v_lr")
        self.clip_ratio, self.target_kl = per_member(clip_ratio, P, "clip_ratio"), per_member(target_kl, P, "target_kl")
        self.max_grad_norm = per_member(max_grad_norm, P, "max_grad_norm", none=0.0)
        if num_mini_batches < 1:
            raise ValueError("num_mini_batches must be at least 1")
        if any(t < 0.0 for t in self.target_kl):
            raise ValueError("target_kl must not be negative: the first step is taken at KL = 0")
        if any(not (lr >= 0.0 and math.isfinite(lr)) for lr in self.pi_lr + self.v_lr) \
                or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not eps >= 0.0:
            raise ValueError(f"invalid Adam hyper-parameters pi_lr={pi_lr} v_lr={v_lr} betas={betas} eps={eps}")
        generators = self._check_generators(generators, P)
        dev = torch.device(pop.device)
        if dev.type != "cuda":
            raise ValueError("PopulationPPOUpdater needs the population on the GPU")
        self.pop, self.generators = pop, generators
        self.train_pi_iterations, self.train_v_iterations = int(train_pi_iterations), int(train_v_iterations)
        self.num_mini_batches = int(num_mini_batches)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        ac = pop.acs[0]
        self.count = flat_slice(ac, "v")[1] + 2 * pop.obs_dim
        self.pi_slice, self.v_slice = flat_slice(ac, "pi"), flat_slice(ac, "v")
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
        self.pi_lr_dev, self.v_lr_dev, self.clip_dev = f32(self.pi_lr), f32(self.v_lr), f32(self.clip_ratio)
        self.target_kl_dev, self.max_grad_norm_dev = f32(self.target_kl), f32(self.max_grad_norm)
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=dev)
        self.flat, self.grad = z(P, self.count), z(P, self.count)
        # the members' DeviceAdam states, [P, ...]: whole blocks, only the slices are ever touched
        self.opt = {w: {"exp_avg": z(P, self.count), "exp_avg_sq": z(P, self.count), "step": z(P, dt=torch.int32),
                        "norm": z(P, dt=torch.float64)} for w in ("pi", "v")}
        self.ctrl = z(P, 4, dt=torch.int32)
        self.summary0, self.summary, self.summary_v, self.summary_mb = (z(P, 8, dt=torch.float64) for _ in range(4))
        self._bufs, self._pending = None, None

    def result(self) -> list | None:
        """The last update's results, one dict of ``ResidentPPOUpdater.KEYS`` per member (one device
        read); None before the first update."""
        from .ppo import ResidentPPOUpdater
        if self._pending is None:
            return None
        out = [dict(zip(ResidentPPOUpdater.KEYS, row)) for row in self._pending.tolist()]
        for o in out:
            o["StopIter"] = int(o["StopIter"])
        return out

    def _buffers(self, rows: int, dev):
        key = (rows, str(dev))
        if self._bufs is None or self._bufs["key"] != key:
            lib, P, d = self.pop.lib, len(self.pop), self.pop.obs_dim
            nbytes = max(lib.cf2_ppo_pop_scratch_bytes(P, rows, d), lib.cf2_column_moments_scratch_bytes(rows, 1))
            self._bufs = {"key": key, "scratch": torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev),
                          "idx": torch.empty(self.train_v_iterations, P, rows, dtype=torch.int32, device=dev),
                          "mu_old": torch.empty(P, rows, 4, device=dev),
                          "moments": torch.empty(P, 2, dtype=torch.float64, device=dev)}
        return self._bufs

    @torch.no_grad()
    def update(self, rollout: PopulationRollout, read: bool = True):
        from . import _native
        pop, lib, p = self.pop, self.pop.lib, _native.ptr
        P, d, dev = len(pop), pop.obs_dim, self.flat.device
        ms, rows, base, stride = self._member_views(rollout)
        B = self._buffers(rows, dev)
        scratch, idx, mu_old, mom = B["scratch"], B["idx"], B["mu_old"], B["moments"]
        flat, grad, ctrl, summary0, summary = self.flat, self.grad, self.ctrl, self.summary0, self.summary
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._begin(ms, rows, idx, mom, scratch, stream)

        def pol(summ, grad=None, mu_old=None, mu_out=None, gate=None):
            _native.check(lib.cf2_ppo_policy_grad_pop(
                P, p(flat), self.count, d, p(base["obs"]), stride["obs"], p(base["act"]), stride["act"], p(base["logp"]),
                stride["logp"], p(base["adv"]), stride["adv"], rows, None, 0, rows, p(mom), p(self.clip_dev), p(mu_old),
                4 * rows, p(mu_out), 4 * rows, None, 0, p(grad), p(summ), p(scratch), p(gate), stream),
                "cf2_ppo_policy_grad_pop")

        val = self._value_call(rows, base, stride, scratch, stream)
        ctrl.zero_()
        summary.zero_()                   # KL and ClipFrac of an update without a policy step
        val(self.summary_v)
        iters = self.train_pi_iterations
        pol(summary0, mu_out=mu_old, grad=grad if iters > 0 else None)
        if iters > 0:
            self._adam("pi", kl_summary=summary0, ctrl=ctrl)
            for _ in range(1, iters):
                pol(summary, grad=grad, mu_old=mu_old, gate=ctrl)
                self._adam("pi", kl_summary=summary, ctrl=ctrl)
            pol(summary, mu_old=mu_old, gate=ctrl)
        self._value_phase(val, idx, rows)
        self._end()
        self._pending = torch.cat([summary0[:, 1:2], self.summary_v[:, 1:2], summary[:, 4:5], summary[:, 3:4],
                                   ctrl[:, 1:2].double(), self.opt["pi"]["norm"][:, None]], dim=1)
        return self.result() if read else None


class PopulationNaturalGradientUpdater(_PopulationUpdaterShared):
    """``NaturalGradientUpdater(device=True)`` (TRPO, NPG) for all members of a ``Population`` at once:
    the launch sequence of one resident update -- the starting gradient G0, conjugate gradients with
    the Fisher-vector products, the step, TRPO's line search or NPG's evaluation, then the value
    phase -- every launch serving the P members (cf2_ppo_policy_grad_pop, cf2_ppo_fisher_vec_pop,
    cf2_ng_cg_init_pop, cf2_ng_cg_step_pop, cf2_ng_direction_pop, cf2_ng_line_search_pop,
    cf2_ppo_value_grad_pop, cf2_adam_step_pop), so an update is a number of launches that does not
    depend on P.  Member k's update is bit for bit the one
    ``NaturalGradientUpdater(pop.acs[k], v_lr[k], target_kl[k], ..., fused=pop.member(k),
    generator=generators[k])`` makes on ``rollout.members[k]`` (tests/test_population_natgrad_gpu.py).

    ``v_lr``, ``target_kl``, ``cg_damping`` and ``max_grad_norm`` are each a scalar or a sequence of P
    values, held in device arrays; ``algorithm``, the iteration counts, ``fvp_stride``, the line
    search's length and decay, the number of mini-batches, the betas and eps are shared.  Every
    member has its own solver state, control block and summaries: a member whose conjugate
    gradients have converged, or whose line search has accepted or given up, is skipped by the later
    launches while the others go on.  ``generators``: as ``PopulationPPOUpdater``'s.

    The row buffers are the rollout's member-major storage, read in place; the Fisher-vector
    products read every ``fvp_stride``-th row through one index list that all members share.
    ``update(rollout, read=False)`` never waits for the GPU; ``result()`` reads the P x 10 results in
    one transfer, one dict of ``NaturalGradientUpdater.KEYS`` per member.  ``state_dict()`` is a list
    of P entries, entry k interchangeable with ``NaturalGradientUpdater.state_dict()`` of the
    stand-alone learner.  The per-member torch plumbing is ``PopulationPPOUpdater``'s."""

    def __init__(self, pop: Population, v_lr, target_kl, algorithm: str = "trpo", cg_iters: int = 10, cg_damping=0.1,
                 fvp_stride: int = 4, line_search_steps: int = 25, line_search_decay: float = 0.8,
                 train_v_iterations: int = 5, num_mini_batches: int = 16, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm=None, generators=None):
        from .ppo import NG_STATE_DOUBLES, flat_slice
        P = len(pop)
        if algorithm not in ("trpo", "npg"):
            raise ValueError(f"algorithm must be 'trpo' or 'npg', got {algorithm!r}")
        self.v_lr, self.target_kl = per_member(v_lr, P, "v_lr"), per_member(target_kl, P, "target_kl")
        self.cg_damping = per_member(cg_damping, P, "cg_damping")
        self.max_grad_norm = per_member(max_grad_norm, P, "max_grad_norm", none=0.0)
        if num_mini_batches < 1 or fvp_stride < 1 or cg_iters < 0 or line_search_steps < 1:
            raise ValueError("num_mini_batches, fvp_stride and line_search_steps must be at least 1, cg_iters at least 0")
        if any(not (t >= 0.0 and math.isfinite(t)) for t in self.target_kl + self.cg_damping) \
                or not 0.0 < line_search_decay <= 1.0:
            raise ValueError("target_kl and cg_damping must not be negative (and finite, for every member), "
                             "line_search_decay must lie in (0, 1]")
        if any(not (lr >= 0.0 and math.isfinite(lr)) for lr in self.v_lr) \
                or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not eps >= 0.0:
            raise ValueError(f"invalid Adam hyper-parameters v_lr={v_lr} betas={betas} eps={eps}")
        generators = self._check_generators(generators, P)
        dev = torch.device(pop.device)
        if dev.type != "cuda":
            raise ValueError("PopulationNaturalGradientUpdater needs the population on the GPU")
        self.pop, self.generators, self.algorithm = pop, generators, algorithm
        self.cg_iters, self.fvp_stride = int(cg_iters), int(fvp_stride)
        self.line_search_steps, self.line_search_decay = int(line_search_steps), float(line_search_decay)
        self.train_v_iterations, self.num_mini_batches = int(train_v_iterations), int(num_mini_batches)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        ac = pop.acs[0]
        self.count = flat_slice(ac, "v")[1] + 2 * pop.obs_dim
        self.pi_slice, self.v_slice = flat_slice(ac, "pi"), flat_slice(ac, "v")
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
        self.v_lr_dev, self.target_kl_dev, self.damping_dev = f32(self.v_lr), f32(self.target_kl), f32(self.cg_damping)
        self.max_grad_norm_dev = f32(self.max_grad_norm)
        self.clip_dev = f32([float("inf")] * P)       # the unclipped surrogate -mean(ratio A)
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=dev)
        self.flat, self.grad = z(P, self.count), z(P, self.count)
        self.work = {k: z(P, self.count) for k in ("b", "x", "r", "p", "z", "step", "old")}
        self.opt = {"v": {"exp_avg": z(P, self.count), "exp_avg_sq": z(P, self.count), "step": z(P, dt=torch.int32),
                          "norm": z(P, dt=torch.float64)}}
        self.ctrl = z(P, 4, dt=torch.int32)
        self.ng_state = z(P, NG_STATE_DOUBLES, dt=torch.float64)
        self.summary0, self.summary, self.summary_v, self.summary_mb, self.summary_f = (
            z(P, 8, dt=torch.float64) for _ in range(5))
        self._bufs, self._pending = None, None

    def result(self) -> list | None:
        """The last update's results, one dict of ``NaturalGradientUpdater.KEYS`` per member (one device
        read); None before the first update."""
        from .ppo import NaturalGradientUpdater
        if self._pending is None:
            return None
        out = [dict(zip(NaturalGradientUpdater.KEYS, row)) for row in self._pending.tolist()]
        for o in out:
            o["AcceptanceStep"] = int(o["AcceptanceStep"])
        return out

    def _buffers(self, rows: int, dev):
        key = (rows, self.fvp_stride, str(dev))
        if self._bufs is None or self._bufs["key"] != key:
            lib, P, d = self.pop.lib, len(self.pop), self.pop.obs_dim
            nbytes = max(lib.cf2_ppo_pop_scratch_bytes(P, rows, d), lib.cf2_column_moments_scratch_bytes(rows, 1))
            self._bufs = {"key": key, "scratch": torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev),
                          "idx": torch.empty(self.train_v_iterations, P, rows, dtype=torch.int32, device=dev),
                          "fvp_idx": torch.arange(0, rows, self.fvp_stride, dtype=torch.int32, device=dev),
                          "mu_old": torch.empty(P, rows, 4, device=dev),
                          "moments": torch.empty(P, 2, dtype=torch.float64, device=dev)}
        return self._bufs

    @torch.no_grad()
    def update(self, rollout: PopulationRollout, read: bool = True):
        from . import _native
        from .ppo import (NG_ACCEPT_STEP, NG_ALPHA, NG_BDOTB, NG_EXPECTED, NG_KL_AFTER, NG_RESIDUAL, NG_STEP_FRAC,
                          NG_XHX)
        pop, lib, p = self.pop, self.pop.lib, _native.ptr
        P, d, dev, count = len(pop), pop.obs_dim, self.flat.device, self.count
        ms, rows, base, stride = self._member_views(rollout)
        B = self._buffers(rows, dev)
        scratch, idx, fidx, mu_old, mom = B["scratch"], B["idx"], B["fvp_idx"], B["mu_old"], B["moments"]
        flat, grad, ctrl, st, W = self.flat, self.grad, self.ctrl, self.ng_state, self.work
        summary0, summary = self.summary0, self.summary
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._begin(ms, rows, idx, mom, scratch, stream)

        def pol(summ, grad=None, mu_old=None, mu_out=None, gate=None):
            _native.check(lib.cf2_ppo_policy_grad_pop(
                P, p(flat), count, d, p(base["obs"]), stride["obs"], p(base["act"]), stride["act"], p(base["logp"]),
                stride["logp"], p(base["adv"]), stride["adv"], rows, None, 0, rows, p(mom), p(self.clip_dev), p(mu_old),
                4 * rows, p(mu_out), 4 * rows, None, 0, p(grad), p(summ), p(scratch), p(gate), stream),
                "cf2_ppo_policy_grad_pop")

        def fvp(vec):             # z = F vec on every fvp_stride-th row: one list for all members
            _native.check(lib.cf2_ppo_fisher_vec_pop(
                P, p(flat), count, d, p(base["obs"]), stride["obs"], rows, p(fidx), 0, fidx.numel(), p(vec), count,
                p(W["z"]), count, p(self.summary_f), p(scratch), None, stream), "cf2_ppo_fisher_vec_pop")

        val = self._value_call(rows, base, stride, scratch, stream)
        p0, p1 = self.pi_slice
        ctrl.zero_()
        val(self.summary_v)
        pol(summary0, mu_out=mu_old, grad=grad)
        _native.check(lib.cf2_ng_cg_init_pop(P, p(grad), p(W["b"]), p(W["x"]), p(W["r"]), p(W["p"]), count, p0, p1 - p0,
                                             p(st), None, stream), "cf2_ng_cg_init_pop")
        for _ in range(self.cg_iters):
            fvp(W["p"])
            _native.check(lib.cf2_ng_cg_step_pop(P, p(W["z"]), p(W["x"]), p(W["r"]), p(W["p"]), count, p0, p1 - p0,
                                                 p(self.damping_dev), p(st), None, stream), "cf2_ng_cg_step_pop")
        fvp(W["x"])
        _native.check(lib.cf2_ng_direction_pop(P, p(W["z"]), p(W["x"]), p(W["b"]), p(W["step"]), p(flat), p(W["old"]), count,
                                               p0, p1 - p0, p(self.damping_dev), p(self.target_kl_dev), p(st), None,
                                               stream), "cf2_ng_direction_pop")
        if self.algorithm == "trpo":
            for j in range(self.line_search_steps):
                pol(summary, mu_old=mu_old, gate=ctrl)
                _native.check(lib.cf2_ng_line_search_pop(
                    P, p(flat), p(W["old"]), p(W["step"]), count, p0, p1 - p0, j, self.line_search_steps,
                    self.line_search_decay, p(self.target_kl_dev), p(summary), summary0.data_ptr() + 8, 8, p(st), p(ctrl),
                    stream), "cf2_ng_line_search_pop")
            after = [st[:, NG_KL_AFTER:NG_KL_AFTER + 1], st[:, NG_ACCEPT_STEP:NG_ACCEPT_STEP + 1],
                     st[:, NG_STEP_FRAC:NG_STEP_FRAC + 1]]
        else:
            pol(summary, mu_old=mu_old)
            one = torch.ones(P, 1, dtype=torch.float64, device=dev)
            after = [summary[:, 4:5], one, one]
        self._value_phase(val, idx, rows)
        self._end()
        self._pending = torch.cat([summary0[:, 1:2], self.summary_v[:, 1:2], after[0], after[1], after[2],
                                   st[:, NG_XHX:NG_XHX + 1], st[:, NG_ALPHA:NG_ALPHA + 1],
                                   st[:, NG_EXPECTED:NG_EXPECTED + 1], st[:, NG_RESIDUAL:NG_RESIDUAL + 1].sqrt(),
                                   st[:, NG_BDOTB:NG_BDOTB + 1].sqrt()], dim=1)
        return self.result() if read else None


__all__ = ["Population", "PopulationMember", "PopulationNaturalGradientUpdater", "PopulationPPOUpdater",
           "PopulationRollout", "collect_population", "member_major", "member_stride", "per_member", "rows_per_member"]
