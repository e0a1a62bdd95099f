"""Populations on the GPU (cf2sim/population.py, csrc/cf2sim_population.hip): P independent learners on
one env batch, every member bit-identical to the run it has alone.  The reference is always the
existing single-policy path -- cf2_policy_forward on the member's rows, ``collect`` on a context of
the member's envs (``env_id_offset = m * n``) with a ``FusedActorCritic`` of the member's seed, the
updaters on a stand-alone learner -- and the comparison is always ``torch.equal``: no tolerances.

Forward shapes (tests/test_population_cpu.py checks without a GPU that the stand-alone reference
is defined for every member's slice of them): P = 3 x 23 rows (two chunks, the second ragged) over
both observation sizes, both precisions, sampled and deterministic; P = 1; P = 64 at the row count
where a member's waves run trips 0..4 of the chunk loop (the noise redrawn at the fifth, half the
waves with a fifth chunk, the last chunk ragged: 4 615 rows per member at 256 CUs); P = 600 members
of 16 rows, more blocks than are resident."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ENV_ID = "DroneHoverBulletFreeEnvWithGust-v0"
FIELDS = ("obs", "act", "rew", "val", "logp", "done", "trunc", "adv", "ret", "last_obs", "last_val", "trunc_val",
          "discounted_ret")
PREC = {"fp32": 0, "bf16x3": 1}
COUNTER, ROW_OFFSET = 5, 1000
SENTINEL = -7.25


def _lib():
    from cf2sim import _native
    return _native.load()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---------------------------------------------------------------- forward, through the Python layer
def _members(gpu, P, d, seed):
    """P modules with distinct random weights, biases, log_std and observation statistics."""
    from cf2sim.rollout import MLPActorCritic
    acs = []
    for m in range(P):
        torch.manual_seed(seed + 17 * m)
        ac = MLPActorCritic(obs_dim=d).to(gpu)
        for mod in ac.modules():
            if isinstance(mod, torch.nn.Linear):
                torch.nn.init.uniform_(mod.bias, -0.3, 0.3)
        ac.obs_oms.update(torch.randn(500, d, device=gpu) * torch.rand(d, device=gpu) * 4 + 1.0)
        with torch.no_grad():
            ac.log_std.copy_(torch.log(torch.rand(4, device=gpu) * 0.8 + 0.1))
        acs.append(ac)
    return acs


def _seeds(P):
    return [((0x9E3779B9 + 977 * m) << 32) | (1234 + m) for m in range(P)]      # both key words in use


@pytest.mark.parametrize("sample", [0, 1])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("obs_dim", [34, 42])
def test_forward_small_equals_each_member_alone(gpu, obs_dim, precision, sample):
    from cf2sim.population import Population
    from cf2sim.rollout import FusedActorCritic
    P, n = 3, 23
    acs, seeds = _members(gpu, P, obs_dim, seed=obs_dim), _seeds(P)
    pop = Population(acs, seeds, precision=precision)
    assert len(pop) == P and _lib().cf2_policy_pop_blocks(P, n) == 1
    g = torch.Generator(device=gpu).manual_seed(3)
    obs = torch.randn(P * n, obs_dim, device=gpu, generator=g) * 3
    act, val, logp = (torch.full(s, SENTINEL, device=gpu) for s in ((P * n, 4), (P * n,), (P * n,)))
    pop.counter = COUNTER
    pop.step_into(obs, act, val, logp, row_offset=ROW_OFFSET, deterministic=not sample)
    assert pop.counter == COUNTER + 1 and pop.member(1).counter == COUNTER + 1
    val2, act2 = torch.full_like(val, SENTINEL), torch.full_like(act, SENTINEL)
    pop.counter = COUNTER
    pop.step_into(obs, act2, val2, None, row_offset=ROW_OFFSET, deterministic=not sample)     # logp_dev NULL
    assert torch.equal(act2, act) and torch.equal(val2, val)
    for m in range(P):
        solo = FusedActorCritic(acs[m], seed=seeds[m], precision=precision)
        assert torch.equal(pop.member(m).w, solo.w), f"member {m}: the population block is not its packed weights"
        assert pop.member(m).seed == solo.seed and pop.member(m).w.data_ptr() == pop.w[m].data_ptr()
        sl = slice(m * n, (m + 1) * n)
        a, v, lp = (torch.empty(s, device=gpu) for s in ((n, 4), (n,), (n,)))
        st = _lib().cf2_policy_forward(solo.w.data_ptr(), n, obs_dim, PREC[precision], obs[sl].data_ptr(), seeds[m],
                                       COUNTER, ROW_OFFSET + n * m, sample, a.data_ptr(), v.data_ptr(), lp.data_ptr(),
                                       _stream(gpu))
        assert st == 0
        for name, got, want in (("act", act[sl], a), ("val", val[sl], v), ("logp", logp[sl], lp)):
            assert torch.equal(got, want), f"member {m} {name}"
    if sample:      # the members draw different noise and differ from a neighbour's weights
        assert not torch.equal(logp[:n], logp[n:2 * n])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("obs_dim", [34, 42])
def test_forward_of_one_member_is_the_single_kernel(gpu, obs_dim, precision):
    from cf2sim.population import Population
    from cf2sim.rollout import FusedActorCritic
    n = 1000
    acs = _members(gpu, 1, obs_dim, seed=7)
    pop = Population(acs, [_seeds(1)[0]], precision=precision)
    solo = FusedActorCritic(acs[0], seed=_seeds(1)[0], precision=precision)
    obs = torch.randn(n, obs_dim, device=gpu, generator=torch.Generator(device=gpu).manual_seed(4)) * 3
    got = [torch.empty(s, device=gpu) for s in ((n, 4), (n,), (n,))]
    want = [torch.empty(s, device=gpu) for s in ((n, 4), (n,), (n,))]
    pop.counter = solo.counter = COUNTER
    pop.step_into(obs, *got, row_offset=ROW_OFFSET)
    solo.step_into(obs, *want, row_offset=ROW_OFFSET)
    for name, a, b in zip(("act", "val", "logp"), got, want):
        assert torch.equal(a, b), name


# ---------------------------------------------------------------- forward, many members (the C ABI)
def _random_flat(gpu, P, d, seed):
    """[P, count] flat weight blocks (the layout of pack_policy_weights): matrices and biases
    N(0, 0.25^2), log_std in log([0.1, 0.9]), observation mean N(0, 1), scale in [0.2, 2.2]."""
    count = _lib().cf2_policy_weights_count(d)
    g = torch.Generator(device=gpu).manual_seed(seed)
    flat = torch.randn(P, count, device=gpu, generator=g) * 0.25
    ls = d * 50 + 50 + 50 * 50 + 50 + 50 * 4 + 4                     # P_LOGSTD of csrc/cf2sim_policy.h
    flat[:, ls:ls + 4] = torch.log(torch.rand(P, 4, device=gpu, generator=g) * 0.8 + 0.1)
    flat[:, count - 2 * d:count - d] = torch.randn(P, d, device=gpu, generator=g)
    flat[:, count - d:] = torch.rand(P, d, device=gpu, generator=g) * 2 + 0.2
    return flat.contiguous()


def _pop_against_members(gpu, P, n, d, precision, seed):
    lib, prec = _lib(), PREC[precision]
    count = lib.cf2_policy_packed_count(d, prec)
    stride = count + 8                                  # a stride above the packed count, still 16-B aligned
    flat = _random_flat(gpu, P, d, seed)
    packed = torch.zeros(P, stride, device=gpu)
    for m in range(P):
        assert lib.cf2_policy_pack(flat[m].data_ptr(), d, prec, packed[m].data_ptr(), _stream(gpu)) == 0
    seeds = _seeds(P)
    seeds_dev = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64, device=gpu)
    obs = torch.randn(P * n, d, device=gpu, generator=torch.Generator(device=gpu).manual_seed(seed + 1)) * 3
    got = [torch.full(s, SENTINEL, device=gpu) for s in ((P * n, 4), (P * n,), (P * n,))]
    want = [torch.full(s, SENTINEL, device=gpu) for s in ((P * n, 4), (P * n,), (P * n,))]
    st = lib.cf2_policy_forward_pop(packed.data_ptr(), stride, P, n, d, prec, obs.data_ptr(), seeds_dev.data_ptr(),
                                    COUNTER, ROW_OFFSET, 1, *[t.data_ptr() for t in got], _stream(gpu))
    assert st == 0
    a_p, v_p, l_p = (t.data_ptr() for t in want)
    for m in range(P):
        r = m * n
        st = lib.cf2_policy_forward(packed[m].data_ptr(), n, d, prec, obs.data_ptr() + r * d * 4, seeds[m], COUNTER,
                                    ROW_OFFSET + r, 1, a_p + r * 16, v_p + r * 4, l_p + r * 4, _stream(gpu))
        assert st == 0, m
    for name, a, b in zip(("act", "val", "logp"), got, want):
        assert not (b == SENTINEL).any(), f"{name}: the reference left rows unwritten"
        if not torch.equal(a, b):
            rows = (a != b).reshape(P * n, -1).any(dim=1).nonzero().flatten()
            raise AssertionError(f"{name}: {rows.numel()} rows differ, first {int(rows[0])} = member {int(rows[0]) // n} "
                                 f"row {int(rows[0]) % n}")


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_forward_every_trip_of_a_members_chunk_loop(gpu, precision):
    """P = 64 at rows = 16 (4 w + w / 2) + 7, w = a member's wave count: trips 0..4 of every member's
    chunk loop, the noise redrawn at the fifth, half the waves with a fifth chunk, the last ragged."""
    lib, P = _lib(), 64
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = b = None
    for cand in range(1, 2 * cus + 1):
        rows = 16 * (4 * 8 * cand + 4 * cand) + 7
        if lib.cf2_policy_pop_blocks(P, rows) == cand:
            n, b = rows, cand
            break
    assert n is not None, "no row count is consistent with cf2_policy_pop_blocks"
    assert b == max(1, min(-(-n // 128), 2 * cus // P))
    kk = (torch.arange(n) // 16) // (8 * b)
    assert int(kk.max()) == 4 and torch.bincount(kk).tolist() == [128 * b] * 4 + [64 * b + 7]
    if cus == 256:
        assert n == 4615 and P * n == 295_360
    _pop_against_members(gpu, P, n, 34, precision, seed=21)


def test_forward_more_members_than_resident_blocks(gpu):
    P, n = 600, 16
    assert _lib().cf2_policy_pop_blocks(P, n) == 1
    assert P > 2 * torch.cuda.get_device_properties(gpu).multi_processor_count
    _pop_against_members(gpu, P, n, 34, "bf16x3", seed=22)


# ---------------------------------------------------------------- collect and training
P_ENV, N_ENV, T = 3, 200, 12
ENV_KW = dict(max_episode_steps=11)      # time-outs at the 11th step of a 12-step collect
ENV_SEED = 11
POLICY_SEEDS = (7, 8, 0xFFFFFFFF00000009)


def _learners(gpu):
    """Three learners with their own weights, standardisation and return statistics.  Members 0 and 1
    push opposite motor pairs apart (a final-layer bias beyond the action clip), so that their
    drones tip over within the time limit; member 2 flies the random policy."""
    from cf2sim.rollout import MLPActorCritic
    acs = []
    for m in range(P_ENV):
        torch.manual_seed(50 + m)
        ac = MLPActorCritic().to(gpu)
        with torch.no_grad():
            ac.obs_oms.mean.uniform_(-0.2, 0.2)
            ac.obs_oms.std.uniform_(0.5, 2.0)
            ac.obs_oms.count.fill_(1000.0)
            ac.ret_oms.std.fill_(2.0 + m)
            ac.ret_oms.count.fill_(1000.0)
            if m < 2:
                ac.pi_net[4].bias.copy_(torch.tensor([[2.0, 2.0, -2.0, -2.0], [2.0, -2.0, -2.0, 2.0]][m], device=gpu))
        acs.append(ac)
    return acs


def _solo_env(m):
    from cf2sim.vec_env import BatchedCrazyflieEnv
    return BatchedCrazyflieEnv(ENV_ID, N_ENV, seed=ENV_SEED, env_id_offset=N_ENV * m, want_final_obs=True, **ENV_KW)


def _pop_env():
    from cf2sim.vec_env import BatchedCrazyflieEnv
    return BatchedCrazyflieEnv(ENV_ID, P_ENV * N_ENV, seed=ENV_SEED, want_final_obs=True, **ENV_KW)


def _check_rollout(tag, got, want):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.shape == b.shape and a.dtype == b.dtype, f"{tag} {f}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
        assert torch.equal(a, b), f"{tag} {f}: max |diff| {(a.float() - b.float()).abs().max().item()}"


def _same_summary(a, b):
    def flat(s):
        return [s["episodes"]] + [s[k][q] for k in ("EpRet", "EpLen") for q in ("mean", "std", "min", "max")]
    fa, fb = flat(a), flat(b)
    return all(x == y or (isinstance(x, float) and math.isnan(x) and math.isnan(y)) for x, y in zip(fa, fb))


@pytest.mark.parametrize("fuse", [False, True])
def test_collect_population_equals_each_member_alone(gpu, fuse):
    from cf2sim.population import Population, collect_population
    from cf2sim.rollout import EpisodeStats, FusedActorCritic, collect
    acs = _learners(gpu)
    pop = Population(acs, POLICY_SEEDS)
    envs = _pop_env()
    stats = [EpisodeStats(N_ENV, gpu) for _ in range(P_ENV)]
    ro = collect_population(envs, pop, T, stats=stats)
    assert ro.last_obs.shape == (P_ENV * N_ENV, 34) and pop.counter == T + 1
    done = torch.stack([r.done for r in ro.members])
    trunc = torch.stack([r.trunc for r in ro.members])
    assert trunc.any(), "no time-out inside the collect"
    assert (done & ~trunc).any(), "no crash inside the collect"
    assert (trunc & ~done).sum() == 0
    ro2 = collect_population(envs, pop, T, obs=ro.last_obs, out=ro, stats=stats)
    assert ro2.storage is ro.storage and pop.counter == 2 * (T + 1)
    assert ro2.members[0].obs.data_ptr() == ro.members[0].obs.data_ptr()       # both storages re-used
    torch.cuda.synchronize()
    # the stand-alone learners; the first population rollout was overwritten by the second, so it
    # is collected again from a fresh population below
    solos = []
    for m in range(P_ENV):
        e, f, st = _solo_env(m), FusedActorCritic(acs[m], seed=POLICY_SEEDS[m]), EpisodeStats(N_ENV, gpu)
        r1 = collect(e, f, T, fuse=fuse, stats=st)
        assert e.last_collect_fused == fuse
        s1 = st.summary(clear=False)
        first = {k: getattr(r1, k).clone() for k in FIELDS}
        r2 = collect(e, f, T, obs=r1.last_obs, fuse=fuse, out=r1, stats=st)
        solos.append((first, s1, r2, st.summary(), f.counter))
        e.close()
    for m in range(P_ENV):
        first, s1, r2, s2, counter = solos[m]
        _check_rollout(f"member {m}, second collect", ro2.members[m], r2)
        assert torch.equal(ro2.last_obs[m * N_ENV:(m + 1) * N_ENV], r2.last_obs)
        assert counter == pop.counter
        assert _same_summary(stats[m].summary(), s2), f"member {m}: episode summary after two collects"
    envs.close()
    # the first collect, from a fresh population and fresh envs
    pop_b, envs_b = Population(acs, POLICY_SEEDS), _pop_env()
    stats_b = [EpisodeStats(N_ENV, gpu) for _ in range(P_ENV)]
    rb = collect_population(envs_b, pop_b, T, stats=stats_b)
    for m in range(P_ENV):
        first, s1 = solos[m][0], solos[m][1]
        for f in FIELDS:
            assert torch.equal(getattr(rb.members[m], f), first[f]), f"member {m}, first collect {f}"
        assert _same_summary(stats_b[m].summary(), s1), f"member {m}: episode summary"
        assert rb.members[m].obs.is_contiguous() and rb.members[m].act.is_contiguous()
    envs_b.close()
    with pytest.raises(ValueError):
        collect_population(_FakeEnvs(601), pop, T)


class _FakeEnvs:
    final_obs = object()

    def __init__(self, n):
        self.num_envs = n


def _stats_of(ac):
    return [t.clone() for oms in (ac.obs_oms, ac.ret_oms) for t in (oms.mean, oms.std, oms.count)]


def test_training_a_population_equals_training_each_member_alone(gpu):
    from cf2sim.population import Population, collect_population
    from cf2sim.ppo import NaturalGradientUpdater, ResidentPPOUpdater
    from cf2sim.rollout import FusedActorCritic, collect, pack_policy_weights, update_running_statistics
    acs_p = _learners(gpu)
    acs_s = [copy.deepcopy(ac) for ac in acs_p]
    gen = lambda m: torch.Generator(device=gpu).manual_seed(100 + m)
    ppo = lambda ac, fused, m: ResidentPPOUpdater(ac, 3e-4, 1e-3, 0.2, 0.01, train_pi_iterations=3, train_v_iterations=1,
                                                  num_mini_batches=4, fused=fused, generator=gen(m))
    pop = Population(acs_p, POLICY_SEEDS)
    envs = _pop_env()
    ups_p = [ppo(acs_p[m], pop.member(m), m) for m in range(P_ENV)]
    solo = []
    for m in range(P_ENV):
        f = FusedActorCritic(acs_s[m], seed=POLICY_SEEDS[m])
        solo.append({"env": _solo_env(m), "fused": f, "up": ppo(acs_s[m], f, m), "ro": None})
    ro = None
    for epoch in range(3):
        # epochs 0 and 1: PPO for every member; epoch 2: TRPO for member 0 alone
        trpo = epoch == 2
        if trpo:
            ng = lambda ac, fused: NaturalGradientUpdater(ac, 1e-3, 0.01, algorithm="trpo", cg_iters=4, line_search_steps=4,
                                                          train_v_iterations=1, num_mini_batches=4, fused=fused,
                                                          generator=gen(9))
            ups_p[0], solo[0]["up"] = ng(acs_p[0], pop.member(0)), ng(acs_s[0], solo[0]["fused"])
        ro = collect_population(envs, pop, T, obs=None if ro is None else ro.last_obs, out=ro)
        for m in range(P_ENV):
            S = solo[m]
            S["ro"] = collect(S["env"], S["fused"], T, obs=None if S["ro"] is None else S["ro"].last_obs, out=S["ro"])
            _check_rollout(f"epoch {epoch} member {m}", ro.members[m], S["ro"])
            if trpo and m > 0:
                continue
            update_running_statistics(acs_p[m], ro.members[m], pop.member(m), device=True)
            update_running_statistics(acs_s[m], S["ro"], S["fused"], device=True)
            res_p, res_s = ups_p[m].update(ro.members[m]), S["up"].update(S["ro"])
            tag = f"epoch {epoch} member {m}"
            assert res_p.keys() == res_s.keys()
            for k in res_p:
                assert res_p[k] == res_s[k] or (math.isnan(res_p[k]) and math.isnan(res_s[k])), f"{tag} {k}: {res_p[k]} vs {res_s[k]}"
            assert torch.equal(ups_p[m].flat, S["up"].flat), f"{tag}: the stepped weight blocks differ"
            assert torch.equal(pack_policy_weights(acs_p[m]), pack_policy_weights(acs_s[m])), f"{tag}: module weights"
            for a, b in zip(_stats_of(acs_p[m]), _stats_of(acs_s[m])):
                assert torch.equal(a, b), f"{tag}: running statistics"
            assert torch.equal(pop.member(m).w, S["fused"].w), f"{tag}: packed blocks"
        for m in range(P_ENV):      # the population block is current: a fresh pack of every member
            fresh = FusedActorCritic(acs_p[m], seed=0)
            assert torch.equal(pop.w[m, :pop.packed_count], fresh.w), f"epoch {epoch} member {m}: stale packed block"
        if epoch == 0:
            start = _learners(gpu)
            for m in range(P_ENV):
                assert not torch.equal(acs_p[m].pi_net[0].weight, start[m].pi_net[0].weight), "the policy did not move"
                assert not torch.equal(acs_p[m].v_net[0].weight, start[m].v_net[0].weight), "the critic did not move"
    assert pop.counter == solo[0]["fused"].counter == 3 * (T + 1)
    envs.close()
    for S in solo:
        S["env"].close()
