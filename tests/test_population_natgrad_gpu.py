"""TRPO / NPG updates of a population on the GPU (cf2_ppo_fisher_vec_pop, cf2_ng_cg_init_pop,
cf2_ng_cg_step_pop, cf2_ng_direction_pop, cf2_ng_line_search_pop,
cf2sim.population.PopulationNaturalGradientUpdater): every member's outputs are the bits of the
stand-alone path (cf2_ppo_fisher_vec, cf2_ng_cg_init, cf2_ng_cg_step, cf2_ng_direction,
cf2_ng_line_search, NaturalGradientUpdater) on the member's slice of the same inputs.  Every
comparison is of bit patterns; there are no tolerances.

Row counts of the Fisher product: those of tests/test_population_update_gpu.py (one block; several
blocks with a ragged last tile; the 512-block cap; more members than resident blocks; one member).
Solver slices: those of tests/test_natural_gradient.py, the policy slice of obs_dim 34 and a short one
that starts off a 16-byte boundary, in blocks 7 000 floats apart."""
import copy
import dataclasses

import pytest
import torch

from test_natural_gradient import CASES as NG_CASES
from test_natural_gradient import SLICES
from test_population_gpu import ENV_SEED, POLICY_SEEDS, _learners, _random_flat
from test_population_update_cpu import blocks
from test_population_update_gpu import CASES, ENV_ID, N_ENV, P_ENV, SENTINEL, T, _same_results, _same_state, ok, same
from test_ppo_update import synthetic_rollout

pytestmark = pytest.mark.gpu


def _lib():
    from cf2sim import _native
    return _native.load()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def q(t):
    return None if t is None else t.data_ptr()


def p_logstd(d):
    return d * 50 + 50 + 50 * 50 + 50 + 50 * 4 + 4              # P_LOGSTD of csrc/cf2sim_policy.h; P_W1 = 0


# ---------------------------------------------------------------- the Fisher product through the C ABI
class FisherRows:
    """P members' weights, directions and observations in buffers whose member strides exceed the
    slices and differ from buffer to buffer; every word between the members holds the sentinel."""

    def __init__(self, gpu, P, n, m, d, seed):
        lib = _lib()
        self.gpu, self.P, self.n, self.m, self.d = gpu, P, n, m, d
        self.count = count = lib.cf2_policy_weights_count(d)
        g = torch.Generator(device=gpu).manual_seed(seed)
        spec = {"w": (count, 5), "vec": (count, 7), "obs": (n * d, 6), "out": (count, 9)}
        self.stride = {k: e + p for k, (e, p) in spec.items()}
        self.buf = {k: torch.full((P, e + p), SENTINEL, device=gpu) for k, (e, p) in spec.items() if k != "out"}
        self.buf["w"][:, :count] = _random_flat(gpu, P, d, seed)
        self.buf["vec"][:, :count] = torch.randn(P, count, device=gpu, generator=g) * 0.3
        self.buf["obs"][:, :n * d] = torch.randn(P, n * d, device=gpu, generator=g) * 1.5 + 0.3
        assert P == 1 or not torch.equal(self.buf["w"][0], self.buf["w"][1])
        assert P == 1 or not torch.equal(self.buf["vec"][0], self.buf["vec"][1])
        self.slice_bytes = lib.cf2_ppo_pop_scratch_bytes(P, m, d) // P
        assert self.slice_bytes % 16 == 0 and self.slice_bytes * P == lib.cf2_ppo_pop_scratch_bytes(P, m, d)
        self.scratch_solo = torch.empty(lib.cf2_ppo_scratch_bytes(m, d) // 8 + 1, dtype=torch.float64, device=gpu)

    def outputs(self):
        f = lambda *s, dt=torch.float32: torch.full(s, SENTINEL, dtype=dt, device=self.gpu)
        return {"out": f(self.P, self.stride["out"]), "summary": f(self.P, 8, dt=torch.float64),
                "scratch": f(self.P, self.slice_bytes // 8, dt=torch.float64)}

    def solo(self, o, idx=None, idx_stride=0, members=None):
        lib, B, S = _lib(), self.buf, self.stride
        for k in (range(self.P) if members is None else members):
            at = lambda name: B[name].data_ptr() + 4 * k * S[name]
            ok(lib.cf2_ppo_fisher_vec(at("w"), self.d, at("obs"), self.n, None if idx is None else idx.data_ptr() + 4 * k * idx_stride,
                                      self.m, at("vec"), o["out"].data_ptr() + 4 * k * S["out"], o["summary"].data_ptr() + 64 * k,
                                      self.scratch_solo.data_ptr(), None, _stream(self.gpu)))

    def pop(self, o, idx=None, idx_stride=0, ctrl=None):
        lib, B, S = _lib(), self.buf, self.stride
        return lib.cf2_ppo_fisher_vec_pop(self.P, q(B["w"]), S["w"], self.d, q(B["obs"]), S["obs"], self.n, q(idx), idx_stride,
                                          self.m, q(B["vec"]), S["vec"], q(o["out"]), S["out"], q(o["summary"]),
                                          q(o["scratch"]), q(ctrl), _stream(self.gpu))

    def check(self, tag, got, want, members=None):
        hi = p_logstd(self.d)
        assert same(got["out"], want["out"]), f"{tag}: out differs from the stand-alone calls"
        assert same(got["summary"], want["summary"]), f"{tag}: summary differs from the stand-alone calls"
        ks = list(range(self.P) if members is None else members)
        o = got["out"][ks]
        assert (o[:, hi:] == SENTINEL).all(), f"{tag}: out written outside [P_W1, P_LOGSTD) or between the members"
        assert (o[:, :hi] != SENTINEL).all(), f"{tag}: the slice is not written"
        s = got["summary"][ks]
        assert (s[:, 0] == self.m).all() and (s[:, 1] > 0).all() and (s[:, 2:] == 0).all(), f"{tag}: summary"
        for t in self.buf.values():          # the inputs' padding is intact
            assert (t[:, -1] == SENTINEL).all()


@pytest.mark.parametrize("d", [34, 42])
@pytest.mark.parametrize("P,m", CASES)
def test_fisher_products_equal_each_member_alone(gpu, P, m, d):
    assert CASES == [(3, 23), (3, 197), (2, 33000), (600, 16), (1, 197)]
    assert [blocks(r) for _, r in CASES] == [1, 4, 512, 1, 4]
    R = FisherRows(gpu, P, m, m, d, seed=2000 + 7 * P + m + d)
    got, want, again = R.outputs(), R.outputs(), R.outputs()
    ok(R.pop(got))
    R.solo(want)
    ok(R.pop(again))
    torch.cuda.synchronize()
    R.check(f"P={P} m={m} d={d}", got, want)
    assert same(got["out"], again["out"]) and same(got["summary"], again["summary"]), "two runs give different bits"


@pytest.mark.parametrize("d", [34, 42])
def test_every_fourth_row_through_a_shared_and_through_per_member_lists(gpu, d):
    P, n, m = 3, 1000, 250
    R = FisherRows(gpu, P, n, m, d, seed=91 + d)
    shared = torch.arange(0, n, 4, dtype=torch.int32, device=gpu)
    assert shared.numel() == m
    got, want = R.outputs(), R.outputs()
    ok(R.pop(got, idx=shared, idx_stride=0))
    R.solo(want, idx=shared, idx_stride=0)
    torch.cuda.synchronize()
    R.check(f"shared list d={d}", got, want)
    # per-member lists, m + 3 words apart: member k takes the rows k, k + 4, ...
    own = torch.full((P, m + 3), 2 ** 31 - 1, dtype=torch.int32, device=gpu)
    own[:, :m] = shared[None, :] + torch.arange(P, dtype=torch.int32, device=gpu)[:, None]
    before = own.clone()
    got2, want2 = R.outputs(), R.outputs()
    ok(R.pop(got2, idx=own, idx_stride=m + 3))
    R.solo(want2, idx=own, idx_stride=m + 3)
    torch.cuda.synchronize()
    R.check(f"per-member lists d={d}", got2, want2)
    assert torch.equal(own, before), "the index lists are only read"
    assert same(got["out"][0], got2["out"][0]) and not same(got["out"][1], got2["out"][1])


@pytest.mark.parametrize("d", [34, 42])
def test_a_gated_member_of_the_fisher_product_is_skipped(gpu, d):
    R = FisherRows(gpu, 3, 197, 197, d, seed=131 + d)
    ctrl = torch.zeros(3, 4, dtype=torch.int32, device=gpu)
    ctrl[1, 0] = 1
    ctrl[1, 1:] = torch.tensor([5, 6, 7], dtype=torch.int32)       # the other words of the block gate nothing
    ctrl[0, 1:] = torch.tensor([1, 2, 3], dtype=torch.int32)
    before = ctrl.clone()
    got, want = R.outputs(), R.outputs()
    ok(R.pop(got, ctrl=ctrl))
    R.solo(want, members=(0, 2))
    torch.cuda.synchronize()
    for name in ("out", "summary", "scratch"):
        assert (got[name][1] == SENTINEL).all(), f"d={d}: the gated member's {name} was written"
    assert (got["scratch"][[0, 2]] != SENTINEL).any(dim=1).all(), "the ungated members used their scratch slices"
    R.check(f"gated d={d}", got, want, members=(0, 2))
    assert torch.equal(ctrl, before), "the launches only read the control blocks"


# ---------------------------------------------------------------- the solver through the C ABI
STRIDE, DAMPING, TARGET_KL = 7000, (0.1, 0.0, 0.25), (0.01, 1.0, 3.0)
VECTORS = ("grad", "b", "x", "r", "p", "z", "step", "w", "old")


def _hyper(gpu):
    return {"damping": torch.tensor(DAMPING, device=gpu), "target_kl": torch.tensor(TARGET_KL, device=gpu)}


def _solver_state(gpu, begin, count):
    """Three members' blocks with the sentinel in every word outside the slice.  Member 1 has a large
    right-hand side and, with damping 0 and F = I, converges in its first CG step."""
    g = torch.Generator(device=gpu).manual_seed(700 + begin + count)
    S = {k: torch.full((3, STRIDE), SENTINEL, device=gpu) for k in VECTORS}
    sl = slice(begin, begin + count)
    S["grad"][:, sl] = torch.randn(3, count, device=gpu, generator=g) * 0.05
    S["grad"][1, sl] = torch.randn(count, device=gpu, generator=g) * 1e4
    S["w"][:, sl] = torch.randn(3, count, device=gpu, generator=g) * 0.25
    S["st"] = torch.full((3, 16), SENTINEL, dtype=torch.float64, device=gpu)
    fisher = torch.rand(3, count, device=gpu, generator=g) + 0.5           # a diagonal F per member
    fisher[1] = 1.0
    return S, fisher, _hyper(gpu)


def _times_f(S, fisher, name, begin, count):
    S["z"][:, begin:begin + count] = fisher * S[name][:, begin:begin + count]


class PopSolver:
    def __init__(self, gpu, begin, count, hyper):
        self.lib, self.s, self.args, self.h = _lib(), _stream(gpu), (STRIDE, begin, count), hyper

    def init(self, S):
        ok(self.lib.cf2_ng_cg_init_pop(3, q(S["grad"]), q(S["b"]), q(S["x"]), q(S["r"]), q(S["p"]), *self.args, q(S["st"]),
                                       None, self.s))

    def step(self, S):
        ok(self.lib.cf2_ng_cg_step_pop(3, q(S["z"]), q(S["x"]), q(S["r"]), q(S["p"]), *self.args, q(self.h["damping"]),
                                       q(S["st"]), None, self.s))

    def direction(self, S):
        ok(self.lib.cf2_ng_direction_pop(3, q(S["z"]), q(S["x"]), q(S["b"]), q(S["step"]), q(S["w"]), q(S["old"]), *self.args,
                                         q(self.h["damping"]), q(self.h["target_kl"]), q(S["st"]), None, self.s))

    def line_search(self, S, trial, total, decay):
        ok(self.lib.cf2_ng_line_search_pop(3, q(S["w"]), q(S["old"]), q(S["step"]), *self.args, trial, total, decay,
                                           q(self.h["target_kl"]), q(S["eval"]), S["summary0"].data_ptr() + 8, 8, q(S["st"]),
                                           q(S["ctrl"]), self.s))


class SoloSolver(PopSolver):
    """The stand-alone calls, member by member, on base + k * stride and the member's own scalars."""

    def _each(self, S, names):
        for k in range(3):
            yield k, [S[n].data_ptr() + 4 * k * STRIDE for n in names], S["st"].data_ptr() + 128 * k

    def init(self, S):
        for k, v, st in self._each(S, ("grad", "b", "x", "r", "p")):
            ok(self.lib.cf2_ng_cg_init(*v, *self.args[1:], st, None, self.s))

    def step(self, S):
        for k, v, st in self._each(S, ("z", "x", "r", "p")):
            ok(self.lib.cf2_ng_cg_step(*v, *self.args[1:], DAMPING[k], st, None, self.s))

    def direction(self, S):
        for k, v, st in self._each(S, ("z", "x", "b", "step", "w", "old")):
            ok(self.lib.cf2_ng_direction(*v, *self.args[1:], DAMPING[k], TARGET_KL[k], st, None, self.s))

    def line_search(self, S, trial, total, decay):
        for k, v, st in self._each(S, ("w", "old", "step")):
            ok(self.lib.cf2_ng_line_search(*v, *self.args[1:], trial, total, decay, TARGET_KL[k], S["eval"].data_ptr() + 64 * k,
                                           S["summary0"].data_ptr() + 64 * k + 8, st, S["ctrl"].data_ptr() + 16 * k, self.s))


def _canaries_intact(S, begin, count, tag):
    for name in VECTORS:
        t = S[name]
        assert (t[:, :begin] == SENTINEL).all() and (t[:, begin + count:] == SENTINEL).all(), f"{tag}: {name} outside the slice"


def _all_same(A, B, tag):
    for name in A:
        assert same(A[name], B[name]), f"{tag}: {name} differs from the stand-alone calls"


@pytest.mark.parametrize("begin,count", SLICES)
def test_conjugate_gradients_and_direction_equal_each_member_alone(gpu, begin, count):
    from cf2sim import ppo
    assert SLICES == ((0, 4504), (3, 63)) and len(set(DAMPING)) == 3 and len(set(TARGET_KL)) == 3
    A, fisher, hyper = _solver_state(gpu, begin, count)
    B = {k: v.clone() for k, v in A.items()}
    pop, solo = PopSolver(gpu, begin, count, hyper), SoloSolver(gpu, begin, count, hyper)
    sl = slice(begin, begin + count)
    pop.init(A)
    solo.init(B)
    _all_same(A, B, "cg_init")
    assert (A["st"][:, ppo.NG_CG_DONE] == 0).all() and (A["st"][:, ppo.NG_BDOTB] > 0).all()
    frozen = None
    for it in range(4):
        _times_f(A, fisher, "p", begin, count)
        _times_f(B, fisher, "p", begin, count)
        pop.step(A)
        solo.step(B)
        _all_same(A, B, f"cg_step {it}")
        st = A["st"]
        assert st[:, ppo.NG_CG_DONE].tolist() == [0.0, 1.0, 0.0], "member 1 alone has converged"
        assert st[:, ppo.NG_CG_STEPS].tolist() == [it + 1.0, 1.0, it + 1.0], "the others go on in the same launches"
        mine = {k: A[k][1].clone() for k in ("x", "r", "p", "st")}
        if frozen is not None:       # a converged member writes nothing afterwards
            assert all(same(mine[k], frozen[k]) for k in mine), f"cg_step {it}: the converged member was written"
        frozen = mine
    assert same(A["p"][1, sl], A["b"][1, sl])
    _times_f(A, fisher, "x", begin, count)
    _times_f(B, fisher, "x", begin, count)
    w0 = A["w"].clone()
    pop.direction(A)
    solo.direction(B)
    torch.cuda.synchronize()
    _all_same(A, B, "direction")
    _canaries_intact(A, begin, count, "after direction")
    assert same(A["old"][:, sl], w0[:, sl]) and not torch.equal(A["w"][:, sl], w0[:, sl])
    alpha = A["st"][:, ppo.NG_ALPHA]
    assert (alpha > 0).all() and len(set(alpha.tolist())) == 3 and (A["st"][:, ppo.NG_XHX] > 0).all()


def _line_search_state(gpu, begin, count, ctrl0, loss, kl):
    g = torch.Generator(device=gpu).manual_seed(900 + begin + count)
    S = {k: torch.full((3, STRIDE), SENTINEL, device=gpu) for k in ("w", "old", "step")}
    sl = slice(begin, begin + count)
    S["old"][:, sl] = torch.randn(3, count, device=gpu, generator=g) * 0.25
    S["step"][:, sl] = torch.randn(3, count, device=gpu, generator=g) * 0.01
    S["w"][:, sl] = S["old"][:, sl] + S["step"][:, sl]
    S["st"] = torch.full((3, 16), SENTINEL, dtype=torch.float64, device=gpu)
    S["ctrl"] = torch.tensor(ctrl0, dtype=torch.int32, device=gpu)
    S["summary0"] = torch.full((3, 8), SENTINEL, dtype=torch.float64, device=gpu)
    S["summary0"][:, 1] = torch.tensor([0.5, -0.25, 0.125], dtype=torch.float64)
    S["eval"] = torch.full((3, 8), SENTINEL, dtype=torch.float64, device=gpu)
    S["eval"][:, 1] = torch.tensor(loss, dtype=torch.float64)
    S["eval"][:, 4] = torch.tensor(kl, dtype=torch.float64)
    return S


def _line_search_both(gpu, begin, count, S, trial, total):
    hyper = _hyper(gpu)
    A, B = S, {k: v.clone() for k, v in S.items()}
    start = {k: v.clone() for k, v in S.items()}
    decay = float(torch.tensor(0.8, dtype=torch.float32))
    PopSolver(gpu, begin, count, hyper).line_search(A, trial, total, decay)
    SoloSolver(gpu, begin, count, hyper).line_search(B, trial, total, decay)
    torch.cuda.synchronize()
    _all_same(A, B, f"line search trial {trial} of {total}")
    for name in ("w", "old", "step"):
        t = A[name]
        assert (t[:, :begin] == SENTINEL).all() and (t[:, begin + count:] == SENTINEL).all(), f"{name} outside the slice"
    for name in ("old", "step", "eval", "summary0"):
        assert same(A[name], start[name]), f"{name} is only read"
    return A, start


@pytest.mark.parametrize("begin,count", SLICES)
def test_line_search_accepts_shrinks_and_skips_in_one_launch(gpu, begin, count):
    """Trial 1 of 5.  Member 0 (target 0.01): loss 0.4 <= 0.5 and KL 0.012 <= 0.015, accepted.  Member 1
    (target 1.0): KL 2.0 > 1.5, rejected, its weights shrink to old + 0.8^2 step.  Member 2: stopped."""
    from cf2sim import ppo
    sl = slice(begin, begin + count)
    S = _line_search_state(gpu, begin, count, [[0, 0, 0, 0], [0, 0, 0, 0], [1, 9, 0, 0]], [0.4, -0.5, 0.0], [0.012, 2.0, 0.0])
    A, start = _line_search_both(gpu, begin, count, S, 1, 5)
    assert A["ctrl"].tolist() == [[1, 2, 0, 0], [0, 0, 0, 0], [1, 9, 0, 0]]
    assert same(A["w"][0], start["w"][0]) and A["st"][0, ppo.NG_ACCEPT_STEP] == 2.0 and A["st"][0, ppo.NG_KL_AFTER] == 0.012
    assert same(A["st"][1], start["st"][1]) and not torch.equal(A["w"][1, sl], start["w"][1, sl])
    frac = float(torch.tensor(0.8, dtype=torch.float32)) ** 2
    assert torch.allclose(A["w"][1, sl], start["old"][1, sl] + frac * start["step"][1, sl], rtol=1e-6, atol=1e-7)
    for name in ("w", "st", "ctrl"):
        assert same(A[name][2], start[name][2]), f"the stopped member's {name} was written"


@pytest.mark.parametrize("begin,count", SLICES)
def test_line_search_at_the_last_trial_restores_the_old_weights(gpu, begin, count):
    """Trial 4 of 5.  Member 0: the loss rose, rejected at the last trial, weights_old comes back bit
    for bit.  Member 1 (target 1.0): KL 1.4 <= 1.5 and the loss fell, accepted.  Member 2: stopped."""
    from cf2sim import ppo
    sl = slice(begin, begin + count)
    S = _line_search_state(gpu, begin, count, [[0, 0, 0, 0], [0, 0, 0, 0], [1, 3, 0, 0]], [0.6, -0.5, 0.0], [0.001, 1.4, 0.0])
    A, start = _line_search_both(gpu, begin, count, S, 4, 5)
    assert A["ctrl"].tolist() == [[1, 0, 0, 0], [1, 5, 0, 0], [1, 3, 0, 0]]
    assert same(A["w"][0, sl], start["old"][0, sl]) and not same(A["w"][0, sl], start["w"][0, sl])
    st = A["st"]
    assert st[0, ppo.NG_ACCEPT_STEP] == 0.0 and st[0, ppo.NG_STEP_FRAC] == 0.0 and st[0, ppo.NG_LOSS_AFTER] == 0.5
    assert st[1, ppo.NG_ACCEPT_STEP] == 5.0 and st[1, ppo.NG_LOSS_AFTER] == -0.5 and same(A["w"][1], start["w"][1])
    for name in ("w", "st", "ctrl"):
        assert same(A[name][2], start[name][2]), f"the stopped member's {name} was written"


# ---------------------------------------------------------------- whole updates
KW = dict(cg_iters=10, fvp_stride=4, line_search_steps=6, train_v_iterations=2, num_mini_batches=3)
V_LR, MAX_NORM = (1e-3, 2e-3, 5e-4), (0.1, None, 0.5)
KL_T, CG_DAMP = (0.01, 1.0, 3.0), (0.1, 0.05, 0.2)


def _envs():
    from cf2sim.vec_env import BatchedCrazyflieEnv
    return BatchedCrazyflieEnv(ENV_ID, P_ENV * N_ENV, seed=ENV_SEED, want_final_obs=True, max_episode_steps=7)


def _solo_updater(ac, fused, k, gen, algorithm, target_kl=KL_T, damping=CG_DAMP, **kw):
    from cf2sim.ppo import NaturalGradientUpdater
    return NaturalGradientUpdater(ac, V_LR[k], target_kl[k], algorithm=algorithm, cg_damping=damping[k],
                                  max_grad_norm=MAX_NORM[k], fused=fused, generator=gen, device=True, **{**KW, **kw})


def _check_member(tag, k, up, solo, pop, pop2, res_p, res_s):
    from cf2sim.rollout import pack_policy_weights
    assert _same_results(res_p, res_s), f"{tag}: {res_p} vs {res_s}"
    assert same(up.flat[k], solo.flat), f"{tag}: the stepped weight blocks differ"
    assert same(pack_policy_weights(pop.acs[k]), pack_policy_weights(pop2.acs[k])), f"{tag}: module weights"
    for a, b in zip(pop.acs[k].parameters(), pop2.acs[k].parameters()):
        assert same(a.data, b.data), f"{tag}: module parameters"
    assert same(pop.w[k], pop2.w[k]), f"{tag}: packed population block"
    assert _same_state(up.state_dict()[k], solo.state_dict()), f"{tag}: value-optimiser state"


@pytest.mark.parametrize("algorithm", ["trpo", "npg"])
def test_population_updates_equal_each_member_alone(gpu, algorithm):
    from cf2sim.population import Population, PopulationNaturalGradientUpdater, collect_population
    from cf2sim.ppo import NaturalGradientUpdater
    from cf2sim.rollout import update_running_statistics
    assert (P_ENV, N_ENV, T) == (3, 200, 8)
    assert all(len(set(v)) == 3 for v in (KL_T, CG_DAMP, V_LR, MAX_NORM))
    acs_p = _learners(gpu)
    acs_s = [copy.deepcopy(ac) for ac in acs_p]
    pop, pop2 = Population(acs_p, POLICY_SEEDS), Population(acs_s, POLICY_SEEDS)
    gen = lambda k: torch.Generator(device=gpu).manual_seed(100 + k)
    gens_s = [gen(k) for k in range(P_ENV)]
    up = PopulationNaturalGradientUpdater(pop, V_LR, KL_T, algorithm=algorithm, cg_damping=CG_DAMP, max_grad_norm=MAX_NORM,
                                          generators=[gen(k) for k in range(P_ENV)], **KW)
    ups = [_solo_updater(acs_s[k], pop2.member(k), k, gens_s[k], algorithm) for k in range(P_ENV)]
    envs, envs2 = _envs(), _envs()
    ro = ro2 = None

    def collect_both():
        nonlocal ro, ro2
        ro = collect_population(envs, pop, T, obs=None if ro is None else ro.last_obs, out=ro)
        ro2 = collect_population(envs2, pop2, T, obs=None if ro2 is None else ro2.last_obs, out=ro2)
        for k in range(P_ENV):
            update_running_statistics(acs_p[k], ro.members[k], pop.member(k), device=True)
            update_running_statistics(acs_s[k], ro2.members[k], pop2.member(k), device=True)

    steps = []
    for epoch in range(2):
        collect_both()
        assert all(same(ro.members[k].adv, ro2.members[k].adv) for k in range(P_ENV))
        res = up.update(ro)
        assert isinstance(res, list) and len(res) == P_ENV and tuple(res[0]) == NaturalGradientUpdater.KEYS
        solo_res = [ups[k].update(ro2.members[k]) for k in range(P_ENV)]
        for k in range(P_ENV):
            _check_member(f"{algorithm} epoch {epoch} member {k}", k, up, ups[k], pop, pop2, res[k], solo_res[k])
        steps.append([r["AcceptanceStep"] for r in solo_res])
        assert all(r["GradNormPi"] > 0 and r["xHx"] > 0 for r in res)
        assert len({r["Alpha"] for r in res}) == 3, "every member has its own step size"
    print(algorithm, "AcceptanceStep of the stand-alone learners per epoch:", steps)
    if algorithm == "npg":
        assert steps == [[1, 1, 1]] * 2
    else:     # measured on an MI355X: [[1, 3, 1], [1, 1, 2]]
        assert all(len(set(s)) >= 2 for s in steps), f"the stand-alone learners stop at different trials: {steps}"
    start = _learners(gpu)
    for k in range(P_ENV):
        assert not torch.equal(acs_p[k].v_net[0].weight, start[k].v_net[0].weight), "the critic did not move"
        if algorithm == "npg" or steps[0][k] > 0 or steps[1][k] > 0:
            assert not torch.equal(acs_p[k].pi_net[0].weight, start[k].pi_net[0].weight), "the policy did not move"
    # member 1 leaves the population: its entry resumes in a fresh stand-alone updater, whose next
    # update is the population's third for that member; this one is enqueued without a host read
    fresh = _solo_updater(acs_s[1], pop2.member(1), 1, gens_s[1], algorithm)
    fresh.load_state_dict(up.state_dict()[1])
    collect_both()
    assert up.update(ro, read=False) is None
    res = up.result()
    _check_member("third update, member 1 resumed alone", 1, up, fresh, pop, pop2, res[1], fresh.update(ro2.members[1]))
    assert all(_same_results(a, b) for a, b in zip(up.result(), res))
    # an entry of the stand-alone updater's loads into the population's list
    sd = up.state_dict()
    sd[1] = fresh.state_dict()
    up.load_state_dict(sd)
    assert _same_state(up.state_dict()[1], fresh.state_dict())
    envs.close()
    envs2.close()


# ---- a synthetic member-major rollout: tests/test_natural_gradient.py's table (synthetic_rollout(3),
# T = 6, N = 40, damping 0.1, stride 4, 10 CG iterations) gives acceptance steps 1, 2, 3 at target KL
# 0.01, 1.0, 3.0
SYN_KL = tuple(NG_CASES[c][0] for c in ("small", "second", "third"))
SYN_KW = dict(line_search_steps=25, train_v_iterations=1)


def _synthetic(gpu, P):
    """(modules, PopulationRollout): P copies of synthetic_rollout(3)'s learner, and its rows P times
    over in member-major buffers (obs with the extra slab collect_population's storage has)."""
    from cf2sim.population import PopulationRollout
    ac, ro = synthetic_rollout(3)
    Tn, n, d = ro.obs.shape
    S = {"obs": torch.zeros(P, Tn + 1, n, d, device=gpu), "act": torch.zeros(P, Tn, n, 4, device=gpu)}
    S.update({k: torch.zeros(P, Tn, n, device=gpu) for k in ("logp", "adv", "ret")})
    rest = {f.name: getattr(ro, f.name).to(gpu) for f in dataclasses.fields(ro)
            if f.name not in S and isinstance(getattr(ro, f.name), torch.Tensor)}
    members = []
    for k in range(P):
        S["obs"][k, :Tn] = ro.obs.to(gpu)
        for name in ("act", "logp", "adv", "ret"):
            S[name][k] = getattr(ro, name).to(gpu)
        members.append(dataclasses.replace(ro, obs=S["obs"][k, :Tn], act=S["act"][k], logp=S["logp"][k], adv=S["adv"][k],
                                           ret=S["ret"][k], **rest))
    return [copy.deepcopy(ac).to(gpu) for _ in range(P)], PopulationRollout(members, rest["last_obs"])


def test_members_stop_at_their_own_trials_inside_shared_launches(gpu):
    from cf2sim.population import Population, PopulationNaturalGradientUpdater
    assert SYN_KL == (0.01, 1.0, 3.0)
    acs_p, ro = _synthetic(gpu, 3)
    acs_s = [copy.deepcopy(ac) for ac in acs_p]
    pop, pop2 = Population(acs_p, POLICY_SEEDS), Population(acs_s, POLICY_SEEDS)
    gen = lambda k: torch.Generator(device=gpu).manual_seed(100 + k)
    damp = (0.1, 0.1, 0.1)
    up = PopulationNaturalGradientUpdater(pop, V_LR, SYN_KL, cg_damping=damp, max_grad_norm=MAX_NORM,
                                          generators=[gen(k) for k in range(3)], **{**KW, **SYN_KW})
    ups = [_solo_updater(acs_s[k], pop2.member(k), k, gen(k), "trpo", target_kl=SYN_KL, damping=damp, **SYN_KW)
           for k in range(3)]
    res = up.update(ro)
    solo_res = [ups[k].update(ro.members[k]) for k in range(3)]
    steps = [r["AcceptanceStep"] for r in solo_res]
    print("AcceptanceStep of the stand-alone learners:", steps)
    assert len(set(steps)) >= 2, f"the stand-alone learners stop at different trials: {steps}"
    assert steps == [1, 2, 3], "the table of tests/test_natural_gradient.py"
    for k in range(3):
        _check_member(f"synthetic member {k}", k, up, ups[k], pop, pop2, res[k], solo_res[k])
    assert [r["AcceptanceStep"] for r in res] == steps
    assert up.ctrl[:, 0].tolist() == [1, 1, 1] and up.ctrl[:, 1].tolist() == steps


class CountingLib:
    """The library object with every cf2_* call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("cf2_"):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def _count_native_calls(gpu, P, algorithm):
    from cf2sim.population import Population, PopulationNaturalGradientUpdater
    acs, ro = _synthetic(gpu, P)
    pop = Population(acs, POLICY_SEEDS[:P])
    up = PopulationNaturalGradientUpdater(pop, 1e-3, 0.01, algorithm=algorithm, **KW)
    counting = CountingLib(pop.lib)
    pop.lib = counting
    for k in range(P):
        pop.member(k).lib = counting
    up.update(ro)
    return counting.calls


@pytest.mark.parametrize("algorithm", ["trpo", "npg"])
def test_native_calls_of_an_update_do_not_depend_on_the_members(gpu, algorithm):
    one, three = _count_native_calls(gpu, 1, algorithm), _count_native_calls(gpu, 3, algorithm)
    plumbing = {"cf2_column_moments", "cf2_policy_pack", "cf2_policy_weights_count"}    # per member, once per update
    launches = lambda c: {k: v for k, v in c.items() if k not in plumbing and not k.endswith("_bytes")}
    assert launches(one) == launches(three), (one, three)
    assert {k: v for k, v in one.items() if k.endswith("_bytes")} == {k: v for k, v in three.items() if k.endswith("_bytes")}
    assert all(name.endswith("_pop") for name in launches(one)), launches(one)
    cg, ls, v = KW["cg_iters"], KW["line_search_steps"], KW["train_v_iterations"] * KW["num_mini_batches"]
    want = {"cf2_ppo_fisher_vec_pop": cg + 1, "cf2_ng_cg_init_pop": 1, "cf2_ng_cg_step_pop": cg, "cf2_ng_direction_pop": 1,
            "cf2_ppo_policy_grad_pop": 1 + (ls if algorithm == "trpo" else 1), "cf2_ppo_value_grad_pop": 1 + v,
            "cf2_adam_step_pop": v}
    if algorithm == "trpo":
        want["cf2_ng_line_search_pop"] = ls
    assert launches(three) == want
    for name in ("cf2_column_moments", "cf2_policy_pack"):
        assert one[name] == 1 and three[name] == 3, name


def test_a_hand_assembled_rollout_is_rejected(gpu):
    from cf2sim.population import Population, PopulationNaturalGradientUpdater, PopulationRollout
    acs, ro = _synthetic(gpu, 3)
    pop = Population(acs, POLICY_SEEDS)
    up = PopulationNaturalGradientUpdater(pop, 1e-3, 0.01, **KW)
    members = list(ro.members)
    members[1] = copy.copy(members[1])
    members[1].adv = members[1].adv.clone()                 # no longer a slice of the member-major storage
    before = [p.detach().clone() for p in acs[0].parameters()]
    with pytest.raises(ValueError, match="equally spaced"):
        up.update(PopulationRollout(members, ro.last_obs))
    with pytest.raises(ValueError, match="members"):
        up.update(PopulationRollout(members[:2], ro.last_obs))
    assert all(torch.equal(a, b) for a, b in zip(before, acs[0].parameters())) and up.result() is None
