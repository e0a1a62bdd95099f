"""Population updates (cf2sim.population.PopulationPPOUpdater; cf2_ppo_policy_grad_pop,
cf2_ppo_value_grad_pop, cf2_adam_step_pop), the checks that need no GPU: the four entry points in the
header, the binding and the library, the status codes of every argument check (all returned before
anything is launched, so the fake pointers are never read), the scratch size, and the argument
handling of the Python class that runs before any device use."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cf2sim.h")
OK, INVALID, UNSUPPORTED = 0, -1, -4
NAMES = ("cf2_ppo_pop_scratch_bytes", "cf2_ppo_policy_grad_pop", "cf2_ppo_value_grad_pop", "cf2_adam_step_pop")


@pytest.fixture(scope="module")
def lib():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    return _native.load()


# ---------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_bound_and_exported(lib):
    from cf2sim import _native
    txt = open(HEADER).read()
    assert re.search(r"^size_t\s+cf2_ppo_pop_scratch_bytes\s*\(uint32_t members, uint32_t m, uint32_t obs_dim\);", txt,
                     flags=re.M)
    for name in NAMES[1:]:
        assert re.search(rf"^int\s+{name}\s*\(uint32_t members,", txt, flags=re.M), name
    syms = os.popen(f"nm -D --defined-only {lib._name}").read()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS, name
        assert re.search(rf"\bT {name}\b", syms), f"{name} not exported"
    assert lib.cf2_ppo_pop_scratch_bytes.restype is ctypes.c_size_t and len(lib.cf2_ppo_pop_scratch_bytes.argtypes) == 3
    for name, nargs in (("cf2_ppo_policy_grad_pop", 29), ("cf2_ppo_value_grad_pop", 19), ("cf2_adam_step_pop", 19)):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
        # the header's parameter list has as many parameters as the binding
        decl = re.search(rf"^int\s+{name}\s*\((.*?)\);", txt, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == nargs, name
    assert lib.cf2_abi_version() == 8


def test_build_keeps_each_side_in_a_unit_with_its_flags():
    """The gradient side is compiled with cf2sim_ppo.hip's flags and the Adam side with
    cf2sim_optim.hip's: they live in those units."""
    from cf2sim import build
    src = lambda f: open(os.path.join(build.SRC_DIR, f)).read()
    assert "cf2_ppo_policy_grad_pop" in src("cf2sim_ppo.hip") and "cf2_ppo_value_grad_pop" in src("cf2sim_ppo.hip")
    assert "cf2_adam_step_pop" in src("cf2sim_optim.hip")
    assert build.SOURCE_FLAGS["cf2sim_ppo.hip"] == ["-fno-slp-vectorize", "-ffp-contract=on"]
    assert build.SOURCE_FLAGS["cf2sim_optim.hip"] == ["-ffp-contract=off"]


def blocks(m):
    """The stand-alone gradient launch's block count."""
    return min(-(-(-(-m // 16)) // 4), 512)


@pytest.mark.parametrize("d", [34, 42])
def test_scratch_is_members_times_the_rounded_stand_alone_size(lib, d):
    for m in (1, 16, 23, 197, 6400, 32768, 33000, 131072, 2 ** 31 - 1):
        one = lib.cf2_ppo_scratch_bytes(m, d)
        assert one > 0
        slice_bytes = (one + 15) // 16 * 16
        for P in (1, 2, 3, 64, 600):
            assert lib.cf2_ppo_pop_scratch_bytes(P, m, d) == P * slice_bytes, (P, m)
        assert lib.cf2_ppo_pop_scratch_bytes(0, m, d) == 0
    for bad in (0, 33, 35, 41, 43, 64):
        assert lib.cf2_ppo_pop_scratch_bytes(3, 100, bad) == 0, bad
    assert lib.cf2_ppo_pop_scratch_bytes(0, 0, d) == 0
    assert lib.cf2_ppo_pop_scratch_bytes(5, 0, d) == 5 * 512 * 8 * 8        # the summaries' partials only


A = 0x7000_0000_0000        # fake device addresses, 16-B aligned: no accepted call below reaches a launch
POL = dict(members=3, weights=A, s_weights=7000, d=34, obs=A + 0x10000, s_obs=2000, act=A + 0x20000, s_act=400,
           logp_old=A + 0x30000, s_logp_old=101, adv=A + 0x40000, s_adv=103, n=50, idx=None, s_idx=0, m=23,
           adv_moments=A + 0x50000, clip=A + 0x51000, mu_old=A + 0x60000, s_mu_old=404, mu_out=A + 0x70000, s_mu_out=408,
           logp_out=A + 0x80000, s_logp_out=107, grad=A + 0x90000, summary=A + 0xA0000, scratch=A + 0xB0000,
           ctrl=A + 0xC0000)
VAL = dict(members=3, weights=A, s_weights=7000, d=34, obs=A + 0x10000, s_obs=2000, target=A + 0x40000, s_target=103,
           n=50, idx=None, s_idx=0, m=23, val_out=A + 0x80000, s_val_out=107, grad=A + 0x90000, summary=A + 0xA0000,
           scratch=A + 0xB0000, ctrl=None)
ADAM = dict(members=4, weights=A, grad=A + 0x10000, exp_avg=A + 0x20000, exp_avg_sq=A + 0x30000, stride=7000, begin=17,
            count=1025, step=A + 0x40000, lr=A + 0x41000, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=A + 0x42000,
            norm_out=A + 0x43000, kl_summary=A + 0x44000, target_kl=A + 0x45000, ctrl=A + 0x46000)


def pol(lib, **kw):
    return lib.cf2_ppo_policy_grad_pop(*{**POL, **kw}.values(), None)


def val(lib, **kw):
    return lib.cf2_ppo_value_grad_pop(*{**VAL, **kw}.values(), None)


def adam(lib, **kw):
    return lib.cf2_adam_step_pop(*{**ADAM, **kw}.values(), None)


def test_nothing_to_do_returns_ok_before_any_launch(lib):
    """members == 0 and m == 0 (count == 0) launch nothing -- there is no device here to launch on."""
    for call in (pol, val):
        assert call(lib, m=0) == OK and call(lib, members=0) == OK and call(lib, m=0, d=42) == OK
        assert call(lib, m=0, weights=None, obs=None, summary=None) == OK         # as the stand-alone calls
    assert adam(lib, members=0) == OK and adam(lib, count=0) == OK
    assert adam(lib, count=0, weights=None) == OK


def test_unsupported_observation_sizes(lib):
    for d in (0, 33, 35, 41, 43, 64):
        for call in (pol, val):
            assert call(lib, d=d) == UNSUPPORTED and call(lib, d=d, m=0) == UNSUPPORTED
            assert call(lib, d=d, members=0) == UNSUPPORTED and call(lib, d=d, weights=None) == UNSUPPORTED
    assert adam(lib, count=2 ** 20 + 1) == UNSUPPORTED and adam(lib, count=2 ** 20, members=0) == OK


def test_null_required_pointers(lib):
    for name in ("weights", "obs", "act", "logp_old", "adv", "clip", "summary", "scratch"):
        assert pol(lib, **{name: None}) == INVALID, name
    for name in ("weights", "obs", "target", "summary", "scratch"):
        assert val(lib, **{name: None}) == INVALID, name
    for name in ("weights", "grad", "exp_avg", "exp_avg_sq", "step", "lr"):
        assert adam(lib, **{name: None}) == INVALID, name
    # the KL stop needs a target for every member; without ctrl or kl_summary none is read
    assert adam(lib, target_kl=None) == INVALID
    assert pol(lib, n=0) == INVALID and val(lib, n=0) == INVALID


def test_misaligned_base_pointers(lib):
    four = ("weights", "logp_old", "adv", "clip", "mu_old", "mu_out", "logp_out", "grad", "ctrl")
    for name in four:
        assert pol(lib, **{name: POL[name] + 2}) == INVALID, name
    for name, off in (("obs", 4), ("act", 4), ("act", 8), ("adv_moments", 4), ("summary", 4), ("scratch", 4)):
        assert pol(lib, **{name: POL[name] + off}) == INVALID, (name, off)
    assert pol(lib, idx=A + 0xD0002, s_idx=50) == INVALID
    for name in ("weights", "target", "val_out", "grad"):
        assert val(lib, **{name: VAL[name] + 2}) == INVALID, name
    for name, off in (("obs", 4), ("summary", 4), ("scratch", 4)):
        assert val(lib, **{name: VAL[name] + off}) == INVALID, (name, off)
    assert val(lib, ctrl=A + 0xC0002) == INVALID and val(lib, idx=A + 0xD0002, s_idx=50) == INVALID
    for name in ("weights", "grad", "exp_avg", "exp_avg_sq", "step", "lr", "max_grad_norm", "target_kl", "ctrl"):
        assert adam(lib, **{name: ADAM[name] + 2}) == INVALID, name
    for name in ("norm_out", "kl_summary"):
        assert adam(lib, **{name: ADAM[name] + 4}) == INVALID, name


def test_misaligned_strides(lib):
    """A stride keeps every member's pointer as aligned as the base: obs rows are read 8 bytes at a
    time (an even stride in floats), act rows 16 (a multiple of 4)."""
    for s in (2001, 1999, 1):
        assert pol(lib, s_obs=s) == INVALID and val(lib, s_obs=s) == INVALID, s
    for s in (401, 402, 403, 1):
        assert pol(lib, s_act=s) == INVALID, s


def test_more_rows_than_there_are_need_an_index_list(lib):
    assert pol(lib, n=22) == INVALID and val(lib, n=22) == INVALID
    assert pol(lib, n=23, m=24) == INVALID and val(lib, n=23, m=24) == INVALID


def test_grid_overflow(lib):
    """members * blocks per member of either launch (gradient: blocks(m); merge: one per 256 words of
    the value slice, 28 at most) must stay below 2^31."""
    assert blocks(32768) == 512 and blocks(23) == 1 and blocks(197) == 4 and blocks(33000) == 512
    for call in (pol, val):
        assert call(lib, members=2 ** 22, n=32768, m=32768) == INVALID
        assert call(lib, members=2 ** 31 - 1, n=50, m=23) == INVALID          # the merge launch's blocks
        assert call(lib, members=2 ** 32 - 1, n=50, m=23) == INVALID
    assert adam(lib, members=2 ** 31) == INVALID and adam(lib, members=2 ** 32 - 1) == INVALID
    assert adam(lib, begin=2 ** 32 - 1000) == INVALID


# ---------------------------------------------------------------- the Python class
def test_hyper_parameters_broadcast_per_member():
    from cf2sim.population import per_member
    assert per_member(3e-4, 3, "pi_lr") == [3e-4] * 3 and per_member(1, 2, "x") == [1.0, 1.0]
    assert per_member([1e-3, 2e-3, 3e-3], 3, "pi_lr") == [1e-3, 2e-3, 3e-3]
    assert per_member((0.1, 0.2), 2, "clip_ratio") == [0.1, 0.2]
    assert per_member(torch.tensor([0.5, 0.25]), 2, "x") == [0.5, 0.25]
    assert per_member(None, 3, "max_grad_norm", none=0.0) == [0.0] * 3
    assert per_member([None, 0.5, None], 3, "max_grad_norm", none=0.0) == [0.0, 0.5, 0.0]
    for bad in ([1.0, 2.0], [1.0] * 4, []):
        with pytest.raises(ValueError, match="a scalar or a sequence of 3"):
            per_member(bad, 3, "pi_lr")
    with pytest.raises(ValueError, match="required"):
        per_member(None, 3, "pi_lr")


class FakePopulation:
    """What PopulationPPOUpdater reads of a Population before it touches the device."""

    def __init__(self, P, device="cpu"):
        from cf2sim.rollout import MLPActorCritic
        self.acs = [MLPActorCritic() for _ in range(P)]
        self.obs_dim, self.device = 34, torch.device(device)

    def __len__(self):
        return len(self.acs)


def test_updater_checks_its_arguments_before_any_device_use():
    from cf2sim.population import PopulationPPOUpdater
    pop = FakePopulation(3)
    good = dict(pi_lr=3e-4, v_lr=1e-3, clip_ratio=0.2, target_kl=0.01)
    for name in ("pi_lr", "v_lr", "clip_ratio", "target_kl", "max_grad_norm"):
        for bad in ([0.1, 0.2], [0.1] * 4):
            with pytest.raises(ValueError, match=f"{name} must be a scalar or a sequence of 3"):
                PopulationPPOUpdater(pop, **{**good, name: bad})
    with pytest.raises(ValueError, match="target_kl must not be negative"):
        PopulationPPOUpdater(pop, **{**good, "target_kl": [0.01, -1e-3, 0.01]})
    with pytest.raises(ValueError, match="target_kl must not be negative"):
        PopulationPPOUpdater(pop, **{**good, "target_kl": -1.0})
    with pytest.raises(ValueError, match="num_mini_batches"):
        PopulationPPOUpdater(pop, **good, num_mini_batches=0)
    with pytest.raises(ValueError, match="Adam"):
        PopulationPPOUpdater(pop, **{**good, "pi_lr": [1e-3, -1e-3, 1e-3]})
    with pytest.raises(ValueError, match="Adam"):
        PopulationPPOUpdater(pop, **{**good, "v_lr": float("inf")})
    with pytest.raises(ValueError, match="generators"):
        PopulationPPOUpdater(pop, **good, generators=[torch.Generator()] * 2)
    # every argument accepted: the next thing the class needs is the GPU
    with pytest.raises(ValueError, match="on the GPU"):
        PopulationPPOUpdater(pop, pi_lr=[1e-3, 2e-3, 3e-3], v_lr=1e-3, clip_ratio=(0.1, 0.2, 0.3), target_kl=[1e9, 0.0, 0.01],
                             max_grad_norm=[None, 0.5, None], generators=[torch.Generator() for _ in range(3)])


def test_member_strides_of_equally_spaced_slices():
    from cf2sim.population import member_stride
    P, T, n, d = 3, 4, 5, 34
    obs = torch.zeros(P, T + 1, n, d)                         # the member-major storage: obs has a slab more
    act = torch.zeros(P, T, n, 4)
    assert member_stride([obs[k, :T] for k in range(P)], "obs") == (T + 1) * n * d
    assert member_stride([act[k] for k in range(P)], "act") == T * n * 4
    assert member_stride([act[1]], "act") == T * n * 4        # one member: its own size
    assert member_stride([obs[k, 1:3] for k in range(P)], "obs") == (T + 1) * n * d


def test_unequally_spaced_member_tensors_raise():
    from cf2sim.population import member_stride
    P, T, n = 3, 4, 5
    adv = torch.zeros(P + 1, T, n)
    with pytest.raises(ValueError, match="equally spaced"):
        member_stride([adv[0], adv[1], adv[3]], "adv")                        # a gap
    with pytest.raises(ValueError, match="equally spaced"):
        member_stride([adv[2], adv[1], adv[0]], "adv")                        # descending
    with pytest.raises(ValueError, match="equally spaced"):
        member_stride([adv[0], adv[0], adv[0]], "adv")                        # one buffer three times
    with pytest.raises(ValueError, match="equally spaced"):
        member_stride([adv[0], adv[2], adv[3]], "adv")                        # two strides
    with pytest.raises(ValueError, match="contiguous tensors of one shape"):
        member_stride([adv[0], adv[1, :3], adv[2]], "adv")                    # another shape
    with pytest.raises(ValueError, match="contiguous tensors of one shape"):
        member_stride([adv[k, :, :4] for k in range(P)], "adv")               # a column slice is not contiguous
    with pytest.raises(ValueError, match="contiguous tensors of one shape"):
        member_stride([adv[0], adv[1].double(), adv[2]], "adv")
    overlapping = torch.zeros(40)
    with pytest.raises(ValueError, match="equally spaced"):
        member_stride([overlapping[4 * k:4 * k + 20].view(T, n) for k in range(P)], "adv")


def test_new_name_is_exported_lazily():
    import cf2sim
    from cf2sim import population
    assert "PopulationPPOUpdater" in cf2sim.__all__ and "PopulationPPOUpdater" in population.__all__
    assert cf2sim.PopulationPPOUpdater is population.PopulationPPOUpdater
    assert "one-launch gradients for all members" not in population.__doc__
