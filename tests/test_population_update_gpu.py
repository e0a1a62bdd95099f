"""Population updates on the GPU (cf2_ppo_policy_grad_pop, cf2_ppo_value_grad_pop, cf2_adam_step_pop,
cf2sim.population.PopulationPPOUpdater): every member's outputs are the bits of the stand-alone path
(cf2_ppo_policy_grad_gated, cf2_ppo_value_grad, cf2_adam_step, ResidentPPOUpdater) on the member's
slice of the same inputs.  Every comparison is of bit patterns; there are no tolerances.

Row counts: the stand-alone gradient launch runs min(ceil(ceil(m / 16) / 4), 512) blocks.  23 rows: one
block, a ragged second tile, two waves without a tile; 197: 13 tiles in 4 blocks, the last with one
tile; 33 000: 2 063 tiles against the 512-block cap, 15 waves taking a second trip; 600 members of 16
rows: more blocks than are resident; one member: the stand-alone call on the same buffers."""
import copy
import math

import pytest
import torch

from test_population_gpu import ENV_SEED, POLICY_SEEDS, _learners, _random_flat
from test_ppo_resident import SLICES, WORDS

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
ENV_ID = "DroneHoverBulletFreeEnvWithGust-v0"


def _lib():
    from cf2sim import _native
    return _native.load()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def ok(status):
    assert status == 0, f"status {status}, hip error {_lib().cf2_last_hip_error()}"


# ---------------------------------------------------------------- gradient calls through the C ABI
class Rows:
    """P members' inputs of the gradient calls in buffers whose member strides exceed the rows and
    differ from buffer to buffer; every word between the members holds the sentinel."""

    def __init__(self, gpu, P, n, m, d, seed, with_idx=False):
        lib = _lib()
        self.gpu, self.P, self.n, self.m, self.d = gpu, P, n, m, d
        self.count = lib.cf2_policy_weights_count(d)
        g = torch.Generator(device=gpu).manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, device=gpu, generator=g)
        # name -> (elements per member, padding): obs strides stay even, act strides multiples of 4
        spec = {"w": (self.count, 5), "obs": (n * d, 6), "act": (n * 4, 8), "logp_old": (n, 3), "adv": (n, 5),
                "ret": (n, 1), "mu_old": (n * 4, 7)}
        self.stride = {k: e + p for k, (e, p) in spec.items()}
        self.buf = {k: torch.full((P, e + p), SENTINEL, device=gpu) for k, (e, p) in spec.items()}
        self.buf["w"][:, :self.count] = _random_flat(gpu, P, d, seed)
        self.buf["obs"][:, :n * d] = rnd(P, n * d) * 1.5 + 0.3
        self.buf["act"][:, :n * 4] = rnd(P, n * 4) * 0.6
        self.buf["adv"][:, :n] = rnd(P, n) * 2.0 + 0.5
        self.buf["ret"][:, :n] = rnd(P, n)
        self.buf["logp_old"][:, :n] = 0.0
        self.buf["mu_old"][:, :n * 4] = 0.0
        a64 = self.buf["adv"][:, :n].double()
        mean = a64.mean(dim=1)
        self.moments = torch.stack([mean, ((a64 - mean[:, None]) ** 2).sum(dim=1)], dim=1).contiguous()
        self.clip = (0.1 + 0.2 * torch.arange(P, device=gpu, dtype=torch.float32) / max(P, 2)).contiguous()
        assert len(set(self.clip.tolist())) == P
        self.idx, self.stride["idx"] = None, 0
        if with_idx:       # each member its own list: repeats, and one index past n (clamped to n - 1)
            self.stride["idx"] = m + 3
            self.idx = torch.full((P, m + 3), 2 ** 31 - 1, dtype=torch.int32, device=gpu)
            self.idx[:, :m] = torch.randint(0, n, (P, m), device=gpu, generator=g, dtype=torch.int32)
            self.idx[:, 7] = self.idx[:, 3]
            self.idx[:, 11] = n + 7
        self.scratch = torch.empty(lib.cf2_ppo_pop_scratch_bytes(P, m, d) // 8 + 1, dtype=torch.float64, device=gpu)
        self.scratch_solo = torch.empty(lib.cf2_ppo_scratch_bytes(m, d) // 8 + 1, dtype=torch.float64, device=gpu)
        # a log-probability near the policy's and means near its means: ratios around 1, a KL that is not 0
        o = self.outputs()
        self.solo_policy(o, grad=False, mu_old=False, mu_out=True, logp_out=True)
        self.buf["logp_old"][:, :n] = o["out"][:, :n] + 0.2 * rnd(P, n) if m == n and not with_idx \
            else o["out"][:, :1].mean() + 0.2 * rnd(P, n)
        if m == n and not with_idx:
            self.buf["mu_old"][:, :4 * n] = o["mu_out"][:, :4 * n] + 0.05 * rnd(P, 4 * n)
        else:
            self.buf["mu_old"][:, :4 * n] = 0.3 * rnd(P, 4 * n)

    def outputs(self):
        P, m = self.P, self.m
        f = lambda *s, dt=torch.float32: torch.full(s, SENTINEL, dtype=dt, device=self.gpu)
        self.out_stride = {"mu_out": 4 * m + 9, "out": m + 1}
        return {"grad": f(P, self.stride["w"]), "mu_out": f(P, 4 * m + 9), "out": f(P, m + 1),
                "summary": f(P, 8, dt=torch.float64)}

    def _p(self, t, stride, k, size=4):
        return None if t is None else t.data_ptr() + size * k * stride

    def solo_policy(self, o, grad, mu_old, mu_out, logp_out, members=None):
        """cf2_ppo_policy_grad_gated member by member on base + k * stride, ungated."""
        lib, B, S = _lib(), self.buf, self.stride
        for k in (range(self.P) if members is None else members):
            p = lambda name: self._p(B[name], S[name], k)
            ok(lib.cf2_ppo_policy_grad_gated(
                p("w"), self.d, p("obs"), p("act"), p("logp_old"), p("adv"), self.n, self._p(self.idx, S["idx"], k), self.m,
                self._p(self.moments, 2, k, 8), float(self.clip[k]), p("mu_old") if mu_old else None,
                self._p(o["mu_out"], self.out_stride["mu_out"], k) if mu_out else None,
                self._p(o["out"], self.out_stride["out"], k) if logp_out else None,
                self._p(o["grad"], S["w"], k) if grad else None, self._p(o["summary"], 8, k, 8),
                self.scratch_solo.data_ptr(), None, _stream(self.gpu)))

    def pop_policy(self, o, grad, mu_old, mu_out, logp_out, ctrl=None):
        lib, B, S = _lib(), self.buf, self.stride
        q = lambda t: None if t is None else t.data_ptr()
        return lib.cf2_ppo_policy_grad_pop(
            self.P, q(B["w"]), S["w"], self.d, q(B["obs"]), S["obs"], q(B["act"]), S["act"], q(B["logp_old"]),
            S["logp_old"], q(B["adv"]), S["adv"], self.n, q(self.idx), S["idx"], self.m, q(self.moments), q(self.clip),
            q(B["mu_old"]) if mu_old else None, S["mu_old"], q(o["mu_out"]) if mu_out else None, self.out_stride["mu_out"],
            q(o["out"]) if logp_out else None, self.out_stride["out"], q(o["grad"]) if grad else None, q(o["summary"]),
            q(self.scratch), q(ctrl), _stream(self.gpu))

    def solo_value(self, o, grad, val_out, members=None):
        lib, B, S = _lib(), self.buf, self.stride
        for k in (range(self.P) if members is None else members):
            p = lambda name: self._p(B[name], S[name], k)
            ok(lib.cf2_ppo_value_grad(
                p("w"), self.d, p("obs"), p("ret"), self.n, self._p(self.idx, S["idx"], k), self.m,
                self._p(o["out"], self.out_stride["out"], k) if val_out else None,
                self._p(o["grad"], S["w"], k) if grad else None, self._p(o["summary"], 8, k, 8),
                self.scratch_solo.data_ptr(), _stream(self.gpu)))

    def pop_value(self, o, grad, val_out, ctrl=None):
        lib, B, S = _lib(), self.buf, self.stride
        q = lambda t: None if t is None else t.data_ptr()
        return lib.cf2_ppo_value_grad_pop(
            self.P, q(B["w"]), S["w"], self.d, q(B["obs"]), S["obs"], q(B["ret"]), S["ret"], self.n, q(self.idx), S["idx"],
            self.m, q(o["out"]) if val_out else None, self.out_stride["out"], q(o["grad"]) if grad else None,
            q(o["summary"]), q(self.scratch), q(ctrl), _stream(self.gpu))


def _check_outputs(tag, got, want, R, slice_name):
    """The whole buffers are equal: the members' results and every word around them."""
    for name in ("grad", "mu_out", "out", "summary"):
        assert same(got[name], want[name]), f"{tag}: {name} differs from the stand-alone calls"
    # and the stand-alone calls wrote what this test means them to: the slice, nothing else
    from test_ppo_update import sizes
    s = sizes(R.d)
    lo, hi = (0, s["pi_end"]) if slice_name == "pi" else (s["v_begin"], s["v_end"])
    g = got["grad"]
    if (g != SENTINEL).any():
        assert (g[:, :lo] == SENTINEL).all() and (g[:, hi:] == SENTINEL).all(), f"{tag}: grad written outside [{lo}, {hi})"
        assert (g[:, lo:hi] != SENTINEL).all(), f"{tag}: grad slice not written"
    assert (got["out"][:, R.m:] == SENTINEL).all() and (got["mu_out"][:, 4 * R.m:] == SENTINEL).all(), f"{tag}: padding"
    assert (got["summary"][:, 0] == R.m).all(), f"{tag}: summary[0] is the row count"


def _gradient_calls_equal_the_stand_alone_calls(R, tag):
    runs = (("policy grad", "pi", dict(grad=True, mu_old=False, mu_out=True, logp_out=True)),
            ("policy grad with KL", "pi", dict(grad=True, mu_old=True, mu_out=False, logp_out=False)),
            ("policy eval", "pi", dict(grad=False, mu_old=True, mu_out=True, logp_out=True)),
            ("value grad", "v", dict(grad=True, val_out=True)),
            ("value eval", "v", dict(grad=False, val_out=False)))
    for name, which, kw in runs:
        got, want = R.outputs(), R.outputs()
        ok((R.pop_policy if which == "pi" else R.pop_value)(got, **kw))
        (R.solo_policy if which == "pi" else R.solo_value)(want, **kw)
        torch.cuda.synchronize()
        _check_outputs(f"{tag} {name}", got, want, R, which)
        if name == "policy grad with KL":
            assert (got["summary"][:, 4] > 0).all(), f"{tag}: the exact KL is exercised"
    for t in R.buf.values():          # the inputs' padding is intact
        assert (t[:, -1] == SENTINEL).all()


CASES = [(3, 23), (3, 197), (2, 33000), (600, 16), (1, 197)]


@pytest.mark.parametrize("d", [34, 42])
@pytest.mark.parametrize("P,m", CASES)
def test_gradient_calls_equal_each_member_alone(gpu, P, m, d):
    from test_population_update_cpu import blocks
    assert [blocks(r) for _, r in CASES] == [1, 4, 512, 1, 4]
    R = Rows(gpu, P, m, m, d, seed=1000 + 7 * P + m + d)
    _gradient_calls_equal_the_stand_alone_calls(R, f"P={P} m={m} d={d}")


@pytest.mark.parametrize("d", [34, 42])
def test_index_lists_per_member(gpu, d):
    R = Rows(gpu, 3, 500, 197, d, seed=77 + d, with_idx=True)
    assert not torch.equal(R.idx[0, :197], R.idx[1, :197]) and (R.idx[:, :197] >= 500).sum() == 3
    _gradient_calls_equal_the_stand_alone_calls(R, f"idx d={d}")


@pytest.mark.parametrize("d", [34, 42])
def test_a_gated_member_is_skipped_and_the_others_are_unaffected(gpu, d):
    R = Rows(gpu, 3, 197, 197, d, seed=31 + d)
    ctrl = torch.zeros(3, 4, dtype=torch.int32, device=gpu)
    ctrl[1, 0] = 1
    ctrl[1, 1:] = torch.tensor([5, 6, 7], dtype=torch.int32)       # the other words of the block gate nothing
    ctrl[0, 1:] = torch.tensor([1, 2, 3], dtype=torch.int32)
    before = ctrl.clone()
    for which, kw in (("pi", dict(grad=True, mu_old=True, mu_out=True, logp_out=True)), ("v", dict(grad=True, val_out=True)),
                      ("pi", dict(grad=False, mu_old=True, mu_out=True, logp_out=True)), ("v", dict(grad=False, val_out=True))):
        got, want = R.outputs(), R.outputs()
        ok((R.pop_policy if which == "pi" else R.pop_value)(got, ctrl=ctrl, **kw))
        (R.solo_policy if which == "pi" else R.solo_value)(want, members=(0, 2), **kw)
        torch.cuda.synchronize()
        for name in ("grad", "mu_out", "out", "summary"):
            assert (got[name][1] == SENTINEL).all(), f"{which} d={d}: the gated member's {name} was written"
            assert same(got[name], want[name]), f"{which} d={d}: {name} of the ungated members"
        assert (got["summary"][[0, 2], 0] == 197).all()
    assert torch.equal(ctrl, before), "the gradient launches only read the control blocks"


# ---------------------------------------------------------------- Adam
def _adam_setup(gpu, begin, count):
    P, stride = 4, WORDS + 3
    g = torch.Generator(device=gpu).manual_seed(500 + begin + count)
    rnd = lambda *s: torch.randn(*s, device=gpu, generator=g)
    S = {"w": rnd(P, stride) * 0.3, "m": rnd(P, stride) * 0.01, "v": rnd(P, stride).abs() * 1e-3,
         "step": torch.tensor([4, 0, 2, 0], dtype=torch.int32, device=gpu),
         "norm": torch.full((P,), SENTINEL, dtype=torch.float64, device=gpu),
         "ctrl": torch.zeros(P, 4, dtype=torch.int32, device=gpu)}
    S["ctrl"][0, 0] = 1                                    # member 0: stopped before the first step
    S["ctrl"][:, 1] = torch.tensor([3, 0, 1, 0], dtype=torch.int32)
    grads = [rnd(P, stride) * 0.05 for _ in range(3)]
    kl = torch.zeros(P, 8, dtype=torch.float64, device=gpu)
    kl[:, 4] = torch.tensor([0.5, 0.5, 1e-3, 0.0], dtype=torch.float64)
    hyper = {"lr": torch.tensor([1e-3, 2e-3, 3e-4, 5e-3], device=gpu),
             "max_grad_norm": torch.tensor([0.0, 0.01, 0.01, 0.0], device=gpu),      # clipping on for members 1 and 2
             "target_kl": torch.tensor([1.0, 0.1, 0.01, 0.01], device=gpu)}          # member 1: 0.5 > 0.1, its flag is set
    sl = slice(begin, begin + count)
    norm2 = float((grads[0][2, sl].double() ** 2).sum()) ** 0.5
    assert count < 10 or norm2 > 0.01, "member 2's steps are clipped"
    return S, grads, kl, hyper, stride


def _adam_pop(gpu, S, grads, kl, hyper, stride, begin, count):
    lib = _lib()
    for g in grads:
        ok(lib.cf2_adam_step_pop(4, S["w"].data_ptr(), g.data_ptr(), S["m"].data_ptr(), S["v"].data_ptr(), stride, begin, count,
                                 S["step"].data_ptr(), hyper["lr"].data_ptr(), 0.9, 0.999, 1e-8,
                                 hyper["max_grad_norm"].data_ptr(), S["norm"].data_ptr(), kl.data_ptr(),
                                 hyper["target_kl"].data_ptr(), S["ctrl"].data_ptr(), _stream(gpu)))


def _adam_solo(gpu, S, grads, kl, hyper, stride, begin, count):
    lib = _lib()
    for g in grads:
        for k in range(4):
            off = 4 * k * stride
            ok(lib.cf2_adam_step(S["w"].data_ptr() + off, g.data_ptr() + off, S["m"].data_ptr() + off, S["v"].data_ptr() + off,
                                 begin, count, S["step"].data_ptr() + 4 * k, float(hyper["lr"][k]), 0.9, 0.999, 1e-8,
                                 float(hyper["max_grad_norm"][k]), S["norm"].data_ptr() + 8 * k, kl.data_ptr() + 64 * k,
                                 float(hyper["target_kl"][k]), S["ctrl"].data_ptr() + 16 * k, _stream(gpu)))


@pytest.mark.parametrize("begin,count", SLICES)
def test_adam_steps_equal_each_member_alone(gpu, begin, count):
    assert [c for _, c in SLICES] == [1, 63, 1025, 6977]
    S0, grads, kl, hyper, stride = _adam_setup(gpu, begin, count)
    clone = lambda S: {k: v.clone() for k, v in S.items()}
    A, B, C = clone(S0), clone(S0), clone(S0)
    _adam_pop(gpu, A, grads, kl, hyper, stride, begin, count)
    _adam_solo(gpu, B, grads, kl, hyper, stride, begin, count)
    _adam_pop(gpu, C, grads, kl, hyper, stride, begin, count)
    torch.cuda.synchronize()
    for name in S0:
        assert same(A[name], B[name]), f"{name} differs from cf2_adam_step member by member"
        assert same(A[name], C[name]), f"{name}: two runs give different bits"
    sl = slice(begin, begin + count)
    # member 0 was stopped, member 1 only had its flag set: nothing else of theirs is written
    for k in (0, 1):
        for name in ("w", "m", "v", "step", "norm"):
            assert same(A[name][k], S0[name][k]), f"member {k} {name}"
    assert A["ctrl"][:, 0].tolist() == [1, 1, 0, 0] and A["ctrl"][:, 1].tolist() == [3, 0, 4, 3]
    assert A["step"].tolist() == [4, 0, 5, 3] and (A["ctrl"][:, 2:] == 0).all()
    for k in (2, 3):      # applied: the slice moved, the words around it did not
        assert not torch.equal(A["w"][k, sl], S0["w"][k, sl])
        for name in ("w", "m", "v"):
            assert same(A[name][k, :begin], S0[name][k, :begin]) and same(A[name][k, begin + count:], S0[name][k, begin + count:])
        assert A["norm"][k] >= 0
    assert float(A["norm"][0]) == SENTINEL and float(A["norm"][1]) == SENTINEL


# ---------------------------------------------------------------- whole updates
P_ENV, N_ENV, T = 3, 200, 8
KW = dict(train_pi_iterations=6, train_v_iterations=2, num_mini_batches=3)
PI_LR, V_LR, CLIP = (3e-4, 1e-3, 3e-3), (1e-3, 2e-3, 5e-4), (0.2, 0.1, 0.3)
TARGET_KL = (1e9, 0.0, 2e-3)
MAX_NORM = (0.1, None, None)


def _envs():
    from cf2sim.vec_env import BatchedCrazyflieEnv
    return BatchedCrazyflieEnv(ENV_ID, P_ENV * N_ENV, seed=ENV_SEED, want_final_obs=True, max_episode_steps=7)


def _solo_updater(ac, fused, k, gen):
    from cf2sim.ppo import ResidentPPOUpdater
    return ResidentPPOUpdater(ac, PI_LR[k], V_LR[k], CLIP[k], TARGET_KL[k], max_grad_norm=MAX_NORM[k], fused=fused,
                              generator=gen, **KW)


def _same_results(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in a)


def _same_state(a, b):
    return a.keys() == b.keys() and all(a[w].keys() == b[w].keys() and all(same(a[w][k], b[w][k]) for k in a[w]) for w in a)


def test_population_updates_equal_each_member_alone(gpu):
    from cf2sim.population import Population, PopulationPPOUpdater, collect_population
    from cf2sim.ppo import ResidentPPOUpdater
    from cf2sim.rollout import pack_policy_weights, update_running_statistics
    acs_p = _learners(gpu)
    acs_s = [copy.deepcopy(ac) for ac in acs_p]
    pop, pop2 = Population(acs_p, POLICY_SEEDS), Population(acs_s, POLICY_SEEDS)
    gen = lambda k: torch.Generator(device=gpu).manual_seed(100 + k)
    gens_s = [gen(k) for k in range(P_ENV)]
    up = PopulationPPOUpdater(pop, PI_LR, V_LR, CLIP, TARGET_KL, max_grad_norm=MAX_NORM,
                              generators=[gen(k) for k in range(P_ENV)], **KW)
    ups = [_solo_updater(acs_s[k], pop2.member(k), k, gens_s[k]) for k in range(P_ENV)]
    envs, envs2 = _envs(), _envs()
    ro = ro2 = None

    def collect_both():
        nonlocal ro, ro2
        ro = collect_population(envs, pop, T, obs=None if ro is None else ro.last_obs, out=ro)
        ro2 = collect_population(envs2, pop2, T, obs=None if ro2 is None else ro2.last_obs, out=ro2)
        for k in range(P_ENV):
            update_running_statistics(acs_p[k], ro.members[k], pop.member(k), device=True)
            update_running_statistics(acs_s[k], ro2.members[k], pop2.member(k), device=True)

    def check_member(tag, k, solo, res_p, res_s):
        assert _same_results(res_p, res_s), f"{tag}: {res_p} vs {res_s}"
        assert same(up.flat[k], solo.flat), f"{tag}: the stepped weight blocks differ"
        assert same(pack_policy_weights(acs_p[k]), pack_policy_weights(acs_s[k])), f"{tag}: module weights"
        for a, b in zip(acs_p[k].parameters(), acs_s[k].parameters()):
            assert same(a.data, b.data), f"{tag}: module parameters"
        assert same(pop.w[k], pop2.w[k]), f"{tag}: packed population block"
        assert _same_state(up.state_dict()[k], solo.state_dict()), f"{tag}: optimiser state"

    stops = []
    for epoch in range(2):
        collect_both()
        assert all(same(ro.members[k].adv, ro2.members[k].adv) for k in range(P_ENV))
        res = up.update(ro)
        assert isinstance(res, list) and len(res) == P_ENV and tuple(res[0]) == ResidentPPOUpdater.KEYS
        for k in range(P_ENV):
            check_member(f"epoch {epoch} member {k}", k, ups[k], res[k], ups[k].update(ro2.members[k]))
        stops.append([r["StopIter"] for r in res])
    assert stops[0][0] == 6 and stops[0][1] == 1, f"the members stop at their own iterations: {stops}"
    assert all(len(set(s)) >= 2 for s in stops), stops
    start = _learners(gpu)
    for k in range(P_ENV):
        assert not torch.equal(acs_p[k].pi_net[0].weight, start[k].pi_net[0].weight), "the policy did not move"
        assert not torch.equal(acs_p[k].v_net[0].weight, start[k].v_net[0].weight), "the critic did not move"
    # member 1 leaves the population: its entry resumes in a fresh stand-alone updater, whose next
    # update is the population's third for that member; this one is enqueued without a host read
    fresh = _solo_updater(acs_s[1], pop2.member(1), 1, gens_s[1])
    fresh.load_state_dict(up.state_dict()[1])
    collect_both()
    assert up.update(ro, read=False) is None
    res = up.result()
    check_member("third update, member 1 resumed alone", 1, fresh, res[1], fresh.update(ro2.members[1]))
    assert up.result() == res or all(_same_results(a, b) for a, b in zip(up.result(), res))
    # an entry of the stand-alone updater's loads into the population's list
    sd = up.state_dict()
    sd[1] = fresh.state_dict()
    up.load_state_dict(sd)
    assert _same_state(up.state_dict()[1], fresh.state_dict())
    envs.close()
    envs2.close()


def test_a_hand_assembled_rollout_is_rejected(gpu):
    from cf2sim.population import Population, PopulationPPOUpdater, PopulationRollout, collect_population
    acs = _learners(gpu)
    pop = Population(acs, POLICY_SEEDS)
    up = PopulationPPOUpdater(pop, 3e-4, 1e-3, 0.2, 0.01, **KW)
    envs = _envs()
    ro = collect_population(envs, pop, T)
    members = list(ro.members)
    members[1] = copy.copy(members[1])
    members[1].adv = members[1].adv.clone()                 # no longer a slice of the member-major storage
    before = [p.detach().clone() for p in acs[0].parameters()]
    with pytest.raises(ValueError, match="equally spaced"):
        up.update(PopulationRollout(members, ro.last_obs))
    with pytest.raises(ValueError, match="members"):
        up.update(PopulationRollout(members[:2], ro.last_obs))
    assert all(torch.equal(a, b) for a, b in zip(before, acs[0].parameters())) and up.result() is None
    envs.close()
