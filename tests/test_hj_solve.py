"""HJ value-table solver, the parts that need no GPU: by-hand known answers and invariants of the
NumPy restatement (tests/hj_solve_reference.py) the kernel is compared with bit for bit, the host-side
time step, the Python model, the table files, and the C ABI's argument checks."""
import ctypes
import math

import numpy as np
import pytest

import hj_solve_reference as ref
from hj_solve_reference import ADV, SHAPE, _axis, hand_rate, small_model, smooth_target
from cf2sim.config import RobotParams, build_config, hj_grid, spec_for_id
from cf2sim.hj_solve import HJModel, parse_levels, save_value_tables, time_step
from cf2sim.vec_env import load_value_tables, value_table_name


@pytest.mark.parametrize("u_mode,d_mode", [("max", "min"), ("min", "max"), ("max", "max")])
@pytest.mark.parametrize("d", range(6))
def test_restatement_known_answer_linear_target(d, u_mode, d_mode):
    """l = x_d: grad l = e_d, so at every node interior along d one tube step gives
    W' - l = dt min(f_d, 0) (d < 3) or dt min(g_d + b_d, 0) (d >= 3), with f, g and b written out by
    hand here.  Pins the strides, the drift's signs and the players' signs without the scheme code.
    Tolerance: the differences of a linear l carry relative rounding of a few ulp of |x_d| / dx <= 8,
    and W' - l cancels |l| <= pi against a change of <= dt |H|: 1e-12 absolute covers both by 100x."""
    model = small_model(1.5, u_mode=u_mode, d_mode=d_mode)
    n = model.shape
    l = np.broadcast_to(_axis(model.nodes(d), d), n).copy()
    dt = 1e-3
    got = ref.step(l, model, dt, tube=True) - l
    hand = hand_rate(model, d)
    want = dt * np.minimum(np.broadcast_to(hand, n), 0.0)
    interior = [slice(None)] * 6
    interior[d] = slice(1, n[d] - 1)
    interior = tuple(interior)
    assert np.abs(got[interior] - want[interior]).max() < 1e-12
    # without the tube's min the players' signs show in every role assignment: W' - l = dt H
    free = ref.step(l, model, dt, tube=False) - l
    want_free = dt * np.broadcast_to(hand, n)
    assert np.abs(free[interior] - want_free[interior]).max() < 1e-12
    assert np.abs(want_free[interior]).max() > 1e-5     # the answer is not trivially zero
    if d < 3 or (u_mode, d_mode) == ("max", "min"):     # (a winning maximiser keeps g + b > 0: the tube stays put)
        assert np.abs(want[interior]).max() > 1e-5


def test_restatement_constant_target_stays_bit_constant():
    model = small_model()
    l = np.full(model.shape, 0.37)
    dt, steps, dt_last = time_step(model, horizon=1.0)
    W, change = ref.solve(l, model, 5, dt, dt_last, tube=True)
    assert np.array_equal(W, l) and change == 0.0
    W, change = ref.solve(l, model, 5, dt, dt_last, tube=False)
    assert np.array_equal(W, l) and change == 0.0


@pytest.mark.parametrize("level", [0.5, 1.5])
def test_restatement_tube_is_below_target_and_non_increasing(level):
    model = small_model(level)
    l = smooth_target(model)
    dt = time_step(model, horizon=1.0)[0]
    hist = []
    W, _ = ref.solve(l, model, 26, dt, 0.5 * dt, tube=True, history=hist)
    prev = l
    for Wk in hist:
        assert (Wk <= prev).all()
        prev = Wk
    assert (W <= l).all() and (W < l).any()
    assert np.isfinite(W).all()


def test_restatement_indexed_step_matches_full_step():
    model = small_model()
    l = smooth_target(model, seed=3)
    dt = time_step(model, horizon=1.0)[0]
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in model.shape], indexing="ij"), axis=-1).reshape(-1, 6)
    for tube in (True, False):
        assert np.array_equal(ref.step_at(l, model, dt, idx, tube), ref.step(l, model, dt, tube).reshape(-1))


@pytest.mark.parametrize("level", [0.0, 0.5, 1.5])
@pytest.mark.parametrize("shape", [SHAPE, (4, 5, 6, 8, 3, 7)])
def test_time_step_against_brute_force(level, shape):
    """dt = cfl / max over every node of sum_d alpha_d / dx_d (the library loops over the distinct
    (phi, theta, p, q, r) combinations in C; the same fp64 expressions, so 4 ulp is generous)."""
    model = small_model(level, shape)
    worst = ref.alpha_sum(model).max()
    for cfl in (0.8, 0.5):
        dt, steps, dt_last = time_step(model, horizon=0.05, cfl=cfl)
        assert abs(dt - cfl / worst) <= 4 * np.spacing(dt)
        assert steps == math.ceil(0.05 / dt) and 0.0 < dt_last <= dt
        assert abs((steps - 1) * dt + dt_last - 0.05) < 1e-15


def test_time_step_lands_on_a_whole_number_of_steps():
    model = small_model()
    dt = time_step(model, horizon=1.0)[0]
    assert time_step(model, horizon=25.5 * dt)[1:] == (26, pytest.approx(0.5 * dt, rel=1e-9))
    assert time_step(model, horizon=24.5 * dt)[1] == 25
    assert time_step(model, horizon=3 * dt)[1] == 3


def test_model_for_config():
    cfg = build_config(ADV, 1)
    m = HJModel.for_config(cfg, 1.5)
    gmin, dx, points = hj_grid()
    robot = RobotParams.from_urdf(spec_for_id(ADV).urdf)
    assert m.shape == (15,) * 6 and m.periodic_mask == 0b000111
    assert m.umax == tuple(cfg.dstb_umax) == (5.3e-3, 5.3e-3, 1.43e-4)
    assert m.dmax == tuple(1.5 * u for u in m.umax)
    assert m.grid_min == tuple(gmin) and m.dx == tuple(dx)
    assert m.inertia == (robot.IXX, robot.IYY, robot.IZZ)
    assert (m.u_mode, m.d_mode) == ("max", "min")      # the step kernel's disturbance decreases V
    for d in range(6):
        assert np.allclose(m.nodes(d), points[d], rtol=0, atol=1e-14)
    assert HJModel.for_config(cfg, 0.5, inertia=(1e-5, 2e-5, 3e-5)).inertia == (1e-5, 2e-5, 3e-5)
    c = m.to_c()
    assert list(c.n) == [15] * 6 and c.u_max_player == 1 and c.d_max_player == 0
    with pytest.raises(ValueError):
        HJModel(u_mode="largest")


def test_package_exports_the_solver_lazily():
    import cf2sim
    from cf2sim import hj_solve
    for name in ("HJModel", "default_target", "time_step", "solve_value_table", "solve_value_tables",
                 "save_value_tables"):
        assert getattr(cf2sim, name) is getattr(hj_solve, name) and name in cf2sim.__all__


def test_parse_levels():
    assert parse_levels("1.5") == [1.5]
    assert parse_levels("0.5,1.5") == [0.5, 1.5]
    got = parse_levels("0.0:3.0:0.1")
    assert len(got) == 31 and got[0] == 0.0 and got[3] == 0.3 and got[-1] == 3.0


def _table(seed):
    return np.random.default_rng(seed).standard_normal(15 ** 6).astype(np.float32).reshape([15] * 6)


def test_saved_tables_load_back_fixed_level(tmp_path):
    cfg = build_config(ADV, 4)                      # level 1.5
    T = _table(1)
    paths = save_value_tables(tmp_path / "tables", {1.5: T, 1.0: _table(2)})
    assert sorted(p.split("/")[-1] for p in paths) == [value_table_name(1.0), value_table_name(1.5)]
    V, tol = load_value_tables(str(tmp_path / "tables"), cfg)
    assert V.shape == (1, 15 ** 6) and np.array_equal(V[0], T.reshape(-1))
    assert tol == [0] * int(cfg.num_levels)


def test_saved_tables_load_back_boltzmann(tmp_path):
    cfg = build_config("DroneHoverBulletFreeEnvWithRandomHJAdversary-v0", 4)
    nl = int(cfg.num_levels)
    levels = [float(cfg.level_values[k]) for k in range(nl)]
    small = np.zeros([15] * 6, np.float32)
    tables = {lv: small + np.float32(k) for k, lv in enumerate(levels)}
    save_value_tables(tmp_path, tables)
    V, tol = load_value_tables(str(tmp_path), cfg)
    assert V.shape == (nl, 15 ** 6) and tol == list(range(nl))
    for k in range(nl):
        assert (V[k] == np.float32(k)).all()


# ---- C ABI: every invalid argument is refused before the device is touched (no GPU here) ----
@pytest.fixture(scope="module")
def lib():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    return _native.load()


W_PTR, TMP_PTR, OUT_PTR, CHG_PTR = 0x10000000, 0x20000000, 0x30000000, 0x40000000   # never dereferenced


def _solve(lib, m, w=W_PTR, tmp=TMP_PTR, steps=3, dt=1e-3, dt_last=1e-3, out=OUT_PTR, chg=CHG_PTR):
    return lib.cf2_hj_solve(ctypes.byref(m) if m is not None else None, w, tmp, steps, dt, dt_last, 1, out, chg, None)


def _bad_models():
    def edit(**kw):
        m = small_model().to_c()
        for name, (k, v) in kw.items():
            getattr(m, name)[k] = v
        return m
    yield "n_d < 3", edit(n=(2, 2))
    yield "n_d = 0", edit(n=(5, 0))
    yield "dx = 0", edit(dx=(1, 0.0))
    yield "dx < 0", edit(dx=(4, -0.1))
    yield "dx nan", edit(dx=(0, float("nan")))
    yield "inertia = 0", edit(inertia=(0, 0.0))
    yield "inertia < 0", edit(inertia=(2, -1e-5))
    yield "umax < 0", edit(umax=(1, -1e-3))
    yield "dmax < 0", edit(dmax=(2, -1e-9))
    big = small_model().to_c()
    for d in range(6):
        big.n[d] = 36                        # 36^6 = 2.18e9 >= 2^31
    yield "2^31 nodes or more", big


def test_abi_rejects_invalid_models(lib):
    from cf2sim._native import CF2_ERR_INVALID_ARG, CF2HJModel
    assert lib.cf2_hj_model_sizeof() == ctypes.sizeof(CF2HJModel)
    dt = ctypes.c_double(-7.0)
    for what, m in _bad_models():
        assert _solve(lib, m) == CF2_ERR_INVALID_ARG, what
        assert lib.cf2_hj_time_step(ctypes.byref(m), 0.8, ctypes.byref(dt)) == CF2_ERR_INVALID_ARG, what
        assert dt.value == -7.0, what
    assert _solve(lib, None) == CF2_ERR_INVALID_ARG
    assert lib.cf2_hj_time_step(None, 0.8, ctypes.byref(dt)) == CF2_ERR_INVALID_ARG
    good = small_model().to_c()
    assert lib.cf2_hj_time_step(ctypes.byref(good), 0.8, None) == CF2_ERR_INVALID_ARG
    assert lib.cf2_hj_time_step(ctypes.byref(good), 0.0, ctypes.byref(dt)) == CF2_ERR_INVALID_ARG
    assert lib.cf2_hj_time_step(ctypes.byref(good), 0.8, ctypes.byref(dt)) == 0 and dt.value > 0.0


def test_abi_rejects_invalid_solve_arguments(lib):
    from cf2sim._native import CF2_ERR_INVALID_ARG, CF2_ERR_UNSUPPORTED
    m = small_model().to_c()
    nbytes = int(np.prod(SHAPE)) * 8
    assert _solve(lib, m, w=None) == CF2_ERR_INVALID_ARG
    assert _solve(lib, m, tmp=None) == CF2_ERR_INVALID_ARG
    assert _solve(lib, m, tmp=W_PTR) == CF2_ERR_INVALID_ARG                     # aliased
    assert _solve(lib, m, tmp=W_PTR + nbytes - 8) == CF2_ERR_INVALID_ARG        # overlapping
    assert _solve(lib, m, out=W_PTR + 16) == CF2_ERR_INVALID_ARG                # the table inside W
    assert _solve(lib, m, out=TMP_PTR) == CF2_ERR_INVALID_ARG
    assert _solve(lib, m, chg=W_PTR + 8) == CF2_ERR_INVALID_ARG
    assert _solve(lib, m, chg=OUT_PTR) == CF2_ERR_INVALID_ARG
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        assert _solve(lib, m, dt=bad) == CF2_ERR_INVALID_ARG
        assert _solve(lib, m, dt_last=bad) == CF2_ERR_INVALID_ARG
    wide = small_model().to_c()
    wide.n[3] = 49                           # valid, but beyond the kernel's per-dimension tables
    assert _solve(lib, wide) == CF2_ERR_UNSUPPORTED
