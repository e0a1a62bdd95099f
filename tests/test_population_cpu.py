"""Populations (cf2sim/population.py, csrc/cf2sim_population.hip), the checks that need no GPU: the
member-major split against naive indexing, the argument errors of the Python layer, the two new
entry points in the header, the binding and the library, the status codes of
cf2_policy_forward_pop's argument checks (all returned before anything is launched, so fake
pointers are never read) and the inputs of the GPU tests' forward shapes."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cf2sim.h")
OK, INVALID, UNSUPPORTED = 0, -1, -4


@pytest.fixture(scope="module")
def lib():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    return _native.load()


# ---------------------------------------------------------------- member-major split
SPLIT_CASES = [  # (T, P, n, trailing shape, dtype): every dtype and rank of the rollout storage
    (13, 3, 5, (34,), torch.float32), (12, 3, 7, (4,), torch.float32), (12, 4, 3, (), torch.float32),
    (5, 2, 9, (), torch.uint8), (5, 7, 1, (), torch.bool), (1, 1, 6, (42,), torch.float32),
    (3, 6, 2, (), torch.int32), (2, 5, 4, (), torch.float64)]


@pytest.mark.parametrize("T,P,n,rest,dtype", SPLIT_CASES)
def test_member_major_equals_naive_indexing(T, P, n, rest, dtype):
    from cf2sim.population import member_major
    g = torch.Generator().manual_seed(T * 100 + P * 10 + n)
    x = torch.randint(0, 200, (T, P * n, *rest), generator=g)
    x = (x % 2).bool() if dtype == torch.bool else x.to(dtype)
    got = member_major(x, P)
    assert got.shape == (P, T, n, *rest) and got.dtype == dtype and got.is_contiguous()
    for m in range(P):
        assert torch.equal(got[m], x[:, m * n:(m + 1) * n])
    # a non-contiguous source (the first T slabs of [T + 1, ...] storage is contiguous; a column slice is not)
    wide = torch.cat([x, x], dim=1)[:, :P * n]
    out = torch.empty_like(got)
    assert member_major(wide, P, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError):
        member_major(x, P, out=torch.empty(P, T, n + 1, *rest, dtype=dtype))


def test_rows_that_do_not_split_raise():
    from cf2sim.population import collect_population, member_major, rows_per_member
    assert rows_per_member(600, 3) == 200 and rows_per_member(7, 7) == 1
    for N, P in ((10, 3), (200, 3), (5, 6), (0, 2), (4, 0)):
        with pytest.raises(ValueError):
            rows_per_member(N, P)
    with pytest.raises(ValueError):
        member_major(torch.zeros(4, 10), 3)

    class ThreeMembers:
        def __len__(self):
            return 3
    envs = types.SimpleNamespace(final_obs=object(), num_envs=601)
    with pytest.raises(ValueError, match="601 rows do not split into 3"):
        collect_population(envs, ThreeMembers(), 4)
    with pytest.raises(ValueError, match="want_final_obs"):
        collect_population(types.SimpleNamespace(final_obs=None, num_envs=600), ThreeMembers(), 4)


def test_population_argument_errors():
    from cf2sim.population import Population
    from cf2sim.rollout import MLPActorCritic
    acs = [MLPActorCritic(), MLPActorCritic(), MLPActorCritic()]
    for seeds in ([1, 2], [1, 2, 3, 4], []):
        with pytest.raises(ValueError, match="3 members need 3 seeds"):
            Population(acs, seeds)
    with pytest.raises(ValueError):
        Population([], [])
    with pytest.raises(ValueError, match="precision"):
        Population(acs, [1, 2, 3], precision="fp16")
    with pytest.raises(ValueError, match="of its own"):
        Population([acs[0], acs[0]], [1, 2])
    with pytest.raises(ValueError, match="one observation size"):
        Population([acs[0], MLPActorCritic(obs_dim=42)], [1, 2])


def test_names_are_exported_lazily():
    import cf2sim
    from cf2sim import population
    for name in ("Population", "PopulationRollout", "collect_population"):
        assert name in cf2sim.__all__ and getattr(cf2sim, name) is getattr(population, name)


# ---------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_bound_and_exported(lib):
    from cf2sim import _native
    txt = open(HEADER).read()
    assert re.search(r"^int\s+cf2_policy_forward_pop\s*\(", txt, flags=re.M)
    assert re.search(r"^uint32_t\s+cf2_policy_pop_blocks\s*\(uint32_t members, uint32_t rows_per_member\);", txt,
                     flags=re.M)
    assert "cf2_policy_forward_pop" in _native.EXPORTED_SYMBOLS
    assert "cf2_policy_pop_blocks" in _native.EXPORTED_SYMBOLS_U32
    syms = os.popen(f"nm -D --defined-only {lib._name}").read()
    for name in ("cf2_policy_forward_pop", "cf2_policy_pop_blocks"):
        assert re.search(rf"\bT {name}\b", syms), f"{name} not exported"
    assert lib.cf2_policy_forward_pop.restype is ctypes.c_int and len(lib.cf2_policy_forward_pop.argtypes) == 15
    assert lib.cf2_policy_pop_blocks.restype is ctypes.c_uint32
    assert lib.cf2_abi_version() == 8


def test_build_gives_the_population_unit_the_policy_units_flags():
    from cf2sim import build
    assert "cf2sim_population.hip" in build.SOURCES
    assert build.SOURCE_FLAGS["cf2sim_population.hip"] == build.SOURCE_FLAGS["cf2sim_policy.hip"] \
        == ["-fno-slp-vectorize", "-ffp-contract=on"]


A = 0x7000_0000_0000        # fake device addresses, 16-B aligned: no accepted call below reaches a launch


def call(lib, packed=A, stride=None, members=3, rows=23, d=34, prec=1, obs=A + 0x1000, seeds=A + 0x2000,
         act=A + 0x3000, val=A + 0x4000, logp=A + 0x5000):
    if stride is None:
        stride = lib.cf2_policy_packed_count(d, prec)
    return lib.cf2_policy_forward_pop(packed, stride, members, rows, d, prec, obs, seeds, 5, 1000, 1, act, val, logp, None)


def test_forward_pop_argument_errors(lib):
    """Every rejected call returns its code without launching (there is no device here to launch on;
    with one, the calls that are accepted below launch nothing either: rows_per_member == 0)."""
    for d, prec in ((34, 0), (34, 1), (42, 0), (42, 1)):
        count = lib.cf2_policy_packed_count(d, prec)
        assert count > 0 and count % 4 == 0
        assert call(lib, d=d, prec=prec, rows=0) == OK
        assert call(lib, d=d, prec=prec, rows=0, logp=None) == OK
        assert call(lib, d=d, prec=prec, rows=0, stride=count + 4) == OK
        for bad in (count - 4, count + 1, count + 2, 0):
            assert call(lib, d=d, prec=prec, rows=0, stride=bad) == INVALID, bad
            assert call(lib, d=d, prec=prec, stride=bad) == INVALID, bad
    for name in ("packed", "obs", "seeds", "act", "val"):
        assert call(lib, **{name: None}) == INVALID, name
        assert call(lib, rows=0, **{name: None}) == INVALID, name
    for name, off in (("obs", 4), ("seeds", 4), ("act", 8), ("packed", 8), ("act", 4), ("packed", 4)):
        base = {"obs": A + 0x1000, "seeds": A + 0x2000, "act": A + 0x3000, "packed": A}[name]
        assert call(lib, **{name: base + off}) == INVALID, (name, off)
    assert call(lib, obs=A + 0x1000 + 8, rows=0) == OK and call(lib, act=A + 0x3000 + 16, rows=0) == OK
    assert call(lib, members=0) == INVALID and call(lib, members=0, rows=0) == INVALID
    for d, prec in ((33, 1), (0, 0), (34, 2), (42, -1), (50, 1)):
        assert call(lib, d=d, prec=prec, stride=70000) == UNSUPPORTED, (d, prec)
        assert call(lib, d=d, prec=prec, stride=70000, rows=0) == UNSUPPORTED, (d, prec)
    # a NULL pointer wins over an unsupported shape, as in cf2_policy_forward
    assert call(lib, d=33, stride=70000, obs=None) == INVALID
    # total rows that do not fit 32 bits
    for members, rows in ((65536, 65536), (2, 2 ** 31), (2 ** 32 - 1, 2), (3, 1431655766)):
        assert members * rows >= 2 ** 32
        assert call(lib, members=members, rows=rows) == INVALID, (members, rows)
        assert lib.cf2_policy_pop_blocks(members, rows) == 0


def test_pop_blocks_without_a_device(lib):
    """The block counts that do not depend on the CU count: rejected arguments give 0, members of at
    most 128 rows one block each."""
    assert lib.cf2_policy_pop_blocks(0, 16) == 0 and lib.cf2_policy_pop_blocks(4, 0) == 0
    assert lib.cf2_policy_pop_blocks(600, 16) == 1 and lib.cf2_policy_pop_blocks(3, 23) == 1
    assert lib.cf2_policy_pop_blocks(1, 128) == 1 and lib.cf2_policy_pop_blocks(2 ** 31 - 1, 2) == 1
    assert lib.cf2_policy_pop_blocks(2 ** 31, 1) == 0       # a grid of 2^31 blocks


# ---------------------------------------------------------------- the GPU tests' forward shapes
def pop_blocks(members, rows, cus):
    """cf2_policy_pop_blocks restated: max(1, min(ceil(rows / 128), floor(2 CUs / members)))."""
    return max(1, min(-(-rows // 128), (2 * cus) // members))


def edge_rows(members, cus):
    """rows = 16 (4 w + w / 2) + 7 with w = 8 blocks(members, rows): a member's waves run four chunks,
    half of them a fifth, the last chunk ragged (the single kernel's edge_rows of
    tests/test_policy_gae_edges.py, per member)."""
    for b in range(1, 2 * cus + 1):
        rows = 16 * (4 * 8 * b + 4 * b) + 7
        if pop_blocks(members, rows, cus) == b:
            return rows, b
    raise AssertionError("no consistent block count")


def test_forward_shapes_are_inputs_the_single_kernel_is_defined_for():
    """Shapes 1-3 of tests/test_population_gpu.py, member by member: the stand-alone reference call
    gets >= 1 row, an observation base that is 8-B aligned (a member's rows start n * D * 4 bytes
    into a 256-B aligned allocation, D * 4 = 136 or 168), an action base that is 16-B aligned and a
    packed base that is 16-B aligned; row_offset + rows stay below 2^32."""
    rows, b = edge_rows(64, 256)
    assert (rows, b) == (4615, 8) and 64 * rows == 295_360
    assert edge_rows(64, 304)[0] == 16 * (4 * 72 + 36) + 7        # another CU count solves too
    chunk = torch.arange(rows) // 16
    kk = chunk // (8 * b)
    assert kk.max() == 4 and torch.bincount(kk).tolist() == [1024] * 4 + [32 * 16 + 7]
    assert torch.unique((chunk % (8 * b))[kk == 4]).tolist() == list(range(33))     # half the waves + the ragged one
    for P, n, dims in ((3, 23, (34, 42)), (1, 1000, (34, 42)), (64, rows, (34,)), (600, 16, (34,))):
        assert n >= 1
        for d in dims:
            for m in range(P):
                assert (m * n * d * 4) % 8 == 0 and (m * n * 4 * 4) % 16 == 0 and (m * n * 4) % 4 == 0
        assert 1000 + P * n < 2 ** 32
    assert (34 * 4, 42 * 4) == (136, 168) and 136 % 8 == 0 and 168 % 8 == 0


def test_packed_stride_keeps_member_blocks_aligned(lib):
    for d in (34, 42):
        for prec in (0, 1):
            count = lib.cf2_policy_packed_count(d, prec)
            stride = (count + 3) // 4 * 4
            assert stride >= count and (stride * 4) % 16 == 0
