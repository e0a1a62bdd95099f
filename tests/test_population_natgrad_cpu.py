"""TRPO / NPG updates of a population (cf2sim.population.PopulationNaturalGradientUpdater;
cf2_ppo_fisher_vec_pop, cf2_ng_cg_init_pop, cf2_ng_cg_step_pop, cf2_ng_direction_pop,
cf2_ng_line_search_pop), the checks that need no GPU: the five entry points in the header, the binding
and the library, the status codes of every argument check (all returned before anything is launched, so
the fake pointers are never read) and the argument handling of the Python class that runs before any
device use."""
import ctypes
import os
import re

import pytest
import torch

from test_population_update_cpu import FakePopulation, blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cf2sim.h")
OK, INVALID, UNSUPPORTED = 0, -1, -4
# name -> parameters in the header
NAMES = {"cf2_ppo_fisher_vec_pop": 18, "cf2_ng_cg_init_pop": 12, "cf2_ng_cg_step_pop": 12, "cf2_ng_direction_pop": 15,
         "cf2_ng_line_search_pop": 17}
TWINS = {"cf2_ppo_fisher_vec_pop": "cf2_ppo_fisher_vec", "cf2_ng_cg_init_pop": "cf2_ng_cg_init",
         "cf2_ng_cg_step_pop": "cf2_ng_cg_step", "cf2_ng_direction_pop": "cf2_ng_direction",
         "cf2_ng_line_search_pop": "cf2_ng_line_search"}


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
    syms = os.popen(f"nm -D --defined-only {lib._name}").read()
    for name, nargs in NAMES.items():
        decl = re.search(rf"^int\s+{name}\s*\((uint32_t members,.*?)\);", txt, flags=re.M | re.S)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == nargs, name
        assert name in _native.EXPORTED_SYMBOLS, name
        assert re.search(rf"\bT {name}\b", syms), f"{name} not exported"
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
        # the comment above the declaration names the stand-alone call it replaces
        head = txt[:decl.start()]
        comment = head[head.rindex("/*"):]
        assert re.search(rf"\b{TWINS[name]}\b(?!_pop)", comment) and "replaces" in comment, name
    assert lib.cf2_abi_version() == 8


def test_new_code_lives_in_the_units_of_its_twins_with_their_flags():
    from cf2sim import build
    src = lambda f: open(os.path.join(build.SRC_DIR, f)).read()
    ppo, ng = src("cf2sim_ppo.hip"), src("cf2sim_natgrad.hip")
    assert 'extern "C" int cf2_ppo_fisher_vec_pop(' in ppo
    for name in list(NAMES)[1:]:
        assert f'extern "C" int {name}(' in ng, name
    # one body serves the stand-alone and the population Fisher kernel
    assert len(re.findall(r"__global__[^;{]*\bppo_fisher_kernel\(", ppo)) == 1
    for kernel in ("ng_cg_init_kernel", "ng_cg_step_kernel", "ng_direction_kernel", "ng_line_search_kernel"):
        assert len(re.findall(rf"__global__[^;{{]*\b{kernel}\(", ng)) == 1, kernel
    assert "atomic" not in ng.lower()
    assert build.SOURCE_FLAGS["cf2sim_ppo.hip"] == ["-fno-slp-vectorize", "-ffp-contract=on"]
    assert build.SOURCE_FLAGS["cf2sim_natgrad.hip"] == ["-ffp-contract=off"]
    assert build.SOURCE_FLAGS["cf2sim_optim.hip"] == ["-ffp-contract=off"]


A = 0x7000_0000_0000        # fake device addresses, 16-B aligned: no accepted call below reaches a launch
FVP = dict(members=3, weights=A, s_weights=7000, d=34, obs=A + 0x10000, s_obs=2000, n=50, idx=None, s_idx=0, m=23,
           vec=A + 0x20000, s_vec=7004, out=A + 0x30000, s_out=7008, summary=A + 0xA0000, scratch=A + 0xB0000,
           ctrl=A + 0xC0000)
INIT = dict(members=3, grad=A, b=A + 0x10000, x=A + 0x20000, r=A + 0x30000, p=A + 0x40000, stride=7000, begin=3, count=63,
            ng_state=A + 0x50000, ctrl=A + 0x60000)
STEP = dict(members=3, z=A, x=A + 0x20000, r=A + 0x30000, p=A + 0x40000, stride=7000, begin=3, count=63,
            damping=A + 0x51000, ng_state=A + 0x50000, ctrl=A + 0x60000)
DIR = dict(members=3, z=A, x=A + 0x20000, b=A + 0x10000, step=A + 0x30000, weights=A + 0x40000, weights_old=A + 0x48000,
           stride=7000, begin=3, count=63, damping=A + 0x51000, target_kl=A + 0x52000, ng_state=A + 0x50000,
           ctrl=A + 0x60000)
LS = dict(members=3, weights=A + 0x40000, weights_old=A + 0x48000, step=A + 0x30000, stride=7000, begin=3, count=63,
          trial=2, total=5, decay=0.8, target_kl=A + 0x52000, eval_summary=A + 0x53000, loss_before=A + 0x54008,
          s_loss_before=8, ng_state=A + 0x50000, ctrl=A + 0x60000)
SOLVER = {"cf2_ng_cg_init_pop": INIT, "cf2_ng_cg_step_pop": STEP, "cf2_ng_direction_pop": DIR, "cf2_ng_line_search_pop": LS}


def fvp(lib, **kw):
    return lib.cf2_ppo_fisher_vec_pop(*{**FVP, **kw}.values(), None)


def solver(lib, name, **kw):
    return getattr(lib, name)(*{**SOLVER[name], **kw}.values(), None)


def test_the_tables_match_the_bindings(lib):
    assert len(FVP) + 1 == NAMES["cf2_ppo_fisher_vec_pop"]
    for name, args in SOLVER.items():
        assert len(args) + 1 == NAMES[name], name


def test_nothing_to_do_returns_ok_before_any_launch(lib):
    """members == 0, m == 0 and count == 0 launch nothing -- there is no device here to launch on."""
    assert fvp(lib, m=0) == OK and fvp(lib, members=0) == OK and fvp(lib, m=0, d=42) == OK
    assert fvp(lib, m=0, weights=None, obs=None, vec=None, out=None, summary=None) == OK     # as the stand-alone call
    for name, args in SOLVER.items():
        assert solver(lib, name, members=0) == OK and solver(lib, name, count=0) == OK, name
        first = list(args)[1]
        assert solver(lib, name, count=0, **{first: None}) == OK, name
        assert solver(lib, name, count=2 ** 20, members=0) == OK, name


def test_unsupported_sizes(lib):
    for d in (0, 33, 35, 41, 43, 64):
        assert fvp(lib, d=d) == UNSUPPORTED and fvp(lib, d=d, m=0) == UNSUPPORTED
        assert fvp(lib, d=d, members=0) == UNSUPPORTED and fvp(lib, d=d, weights=None) == UNSUPPORTED
    for name in SOLVER:
        assert solver(lib, name, count=2 ** 20 + 1) == UNSUPPORTED, name
        assert solver(lib, name, begin=0, count=2 ** 20 + 1) == UNSUPPORTED, name


def test_null_required_pointers(lib):
    for name in ("weights", "obs", "vec", "out", "summary", "scratch"):
        assert fvp(lib, **{name: None}) == INVALID, name
    assert fvp(lib, ctrl=None, members=0) == OK             # the gate is optional
    required = {"cf2_ng_cg_init_pop": ("grad", "b", "x", "r", "p", "ng_state"),
                "cf2_ng_cg_step_pop": ("z", "x", "r", "p", "damping", "ng_state"),
                "cf2_ng_direction_pop": ("z", "x", "b", "step", "weights", "weights_old", "damping", "target_kl", "ng_state"),
                "cf2_ng_line_search_pop": ("weights", "weights_old", "step", "target_kl", "eval_summary", "loss_before",
                                           "ng_state", "ctrl")}
    for name, args in required.items():
        for a in args:
            assert solver(lib, name, **{a: None}) == INVALID, (name, a)
    assert solver(lib, "cf2_ng_line_search_pop", ctrl=None) == INVALID, "the line search writes the stop flag"
    assert fvp(lib, n=0) == INVALID


def test_misaligned_base_pointers(lib):
    for name in ("weights", "vec", "out", "ctrl"):
        assert fvp(lib, **{name: FVP[name] + 2}) == INVALID, name
    for name, off in (("obs", 4), ("summary", 4), ("scratch", 4)):
        assert fvp(lib, **{name: FVP[name] + off}) == INVALID, (name, off)
    assert fvp(lib, idx=A + 0xD0002, s_idx=50) == INVALID and fvp(lib, idx=A + 0xD0002, s_idx=0) == INVALID
    eight = ("ng_state", "eval_summary", "loss_before")
    for name, args in SOLVER.items():
        for a, v in args.items():
            if not isinstance(v, int) or v < A:
                continue
            off = 4 if a in eight else 2
            assert solver(lib, name, **{a: v + off}) == INVALID, (name, a)


def test_misaligned_strides(lib):
    """An obs stride keeps every member's rows 8-byte aligned: an even number of floats."""
    for s in (2001, 1999, 1):
        assert fvp(lib, s_obs=s) == INVALID, s


def test_more_rows_than_there_are_need_an_index_list(lib):
    assert fvp(lib, n=22) == INVALID and fvp(lib, n=23, m=24) == INVALID


def test_grid_overflow_and_slices_past_32_bits(lib):
    assert blocks(32768) == 512 and blocks(23) == 1
    assert fvp(lib, members=2 ** 22, n=32768, m=32768) == INVALID
    assert fvp(lib, members=2 ** 31 - 1, n=50, m=23) == INVALID              # the merge launch's blocks
    assert fvp(lib, members=2 ** 32 - 1, n=50, m=23) == INVALID
    for name in SOLVER:
        assert solver(lib, name, members=2 ** 31) == INVALID and solver(lib, name, members=2 ** 32 - 1) == INVALID, name
        assert solver(lib, name, begin=2 ** 32 - 60) == INVALID, name
        assert solver(lib, name, begin=2 ** 32 - 1, count=1) == INVALID, name


def test_line_search_arguments(lib):
    ls = lambda **kw: solver(lib, "cf2_ng_line_search_pop", **kw)
    for decay in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert ls(decay=decay) == INVALID, decay
    assert ls(trial=5) == INVALID and ls(trial=6) == INVALID and ls(trial=0, total=0) == INVALID
    # accepted values reach the next check: a slice that is too long is what stops these calls
    assert ls(decay=1.0, count=2 ** 20 + 1) == UNSUPPORTED and ls(trial=4, count=2 ** 20 + 1) == UNSUPPORTED


# ---------------------------------------------------------------- the Python class
GOOD = dict(v_lr=1e-3, target_kl=0.01)


def test_updater_checks_its_arguments_before_any_device_use():
    from cf2sim.population import PopulationNaturalGradientUpdater as Up
    pop = FakePopulation(3)
    for name in ("v_lr", "target_kl", "cg_damping", "max_grad_norm"):
        for bad in ([0.1, 0.2], [0.1] * 4):
            with pytest.raises(ValueError, match=f"{name} must be a scalar or a sequence of 3"):
                Up(pop, **{**GOOD, name: bad})
    for name in ("target_kl", "cg_damping"):
        for bad in ([0.01, -1e-3, 0.01], -1.0, [0.01, 0.01, float("nan")]):
            with pytest.raises(ValueError, match="target_kl and cg_damping must not be negative"):
                Up(pop, **{**GOOD, name: bad})
    with pytest.raises(ValueError, match="line_search_decay"):
        Up(pop, **GOOD, line_search_decay=0.0)
    with pytest.raises(ValueError, match="line_search_decay"):
        Up(pop, **GOOD, line_search_decay=1.5)
    for algorithm in ("ppo", "TRPO", None, ["trpo", "npg", "trpo"]):
        with pytest.raises(ValueError, match="algorithm must be 'trpo' or 'npg'"):
            Up(pop, **GOOD, algorithm=algorithm)
    for kw in (dict(num_mini_batches=0), dict(fvp_stride=0), dict(cg_iters=-1), dict(line_search_steps=0)):
        with pytest.raises(ValueError, match="at least"):
            Up(pop, **GOOD, **kw)
    with pytest.raises(ValueError, match="Adam"):
        Up(pop, **{**GOOD, "v_lr": [1e-3, -1e-3, 1e-3]})
    with pytest.raises(ValueError, match="Adam"):
        Up(pop, **{**GOOD, "v_lr": float("inf")})
    with pytest.raises(ValueError, match="Adam"):
        Up(pop, **GOOD, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="generators"):
        Up(pop, **GOOD, generators=[torch.Generator()] * 2)
    with pytest.raises(ValueError, match="generators"):
        Up(pop, **GOOD, generators=[torch.Generator(), 1, torch.Generator()])
    # every argument accepted: the next thing the class needs is the GPU
    for algorithm in ("trpo", "npg"):
        with pytest.raises(ValueError, match="on the GPU"):
            Up(pop, v_lr=[1e-3, 2e-3, 3e-3], target_kl=[0.01, 0.0, 3.0], cg_damping=(0.1, 0.0, 0.3), algorithm=algorithm,
               max_grad_norm=[None, 0.5, None], generators=[torch.Generator() for _ in range(3)])


def test_new_name_is_exported_lazily():
    import cf2sim
    from cf2sim import population
    name = "PopulationNaturalGradientUpdater"
    assert name in cf2sim.__all__ and name in population.__all__
    assert cf2sim.PopulationNaturalGradientUpdater is population.PopulationNaturalGradientUpdater
    assert "TRPO / NPG updates of a population" not in population.__doc__
    # the two updaters share their value phase and plumbing
    ppo, ng = population.PopulationPPOUpdater, population.PopulationNaturalGradientUpdater
    for method in ("_value_phase", "_begin", "_end", "_adam", "_member_views", "state_dict", "load_state_dict"):
        assert getattr(ppo, method) is getattr(ng, method), method
