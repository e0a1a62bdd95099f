"""HJ value-table solver on the GPU (cf2_hj_solve): the fp64 state against the NumPy restatement
(tests/hj_solve_reference.py) bit for bit, the by-hand known answers on the kernel, the change
output, the fp32 table, one full-size step, and a solved table driving the HJ disturbance and an env."""
import math

import numpy as np
import pytest
import torch

import hj_solve_reference as ref
from hj_solve_reference import ADV, SHAPE, _axis, hand_rate, small_model, smooth_target
from cf2sim.config import build_config
from cf2sim.hj_solve import HJModel, default_target, solve_value_table, solve_value_tables, time_step

pytestmark = pytest.mark.gpu

SHAPES = {"mixed": SHAPE, "rates_permuted": (4, 5, 6, 8, 3, 7)}


def _base_dt(model):
    return time_step(model, horizon=1.0)[0]


@pytest.mark.parametrize("nsteps", [26, 25])          # even and odd: the result's ping-pong parity
@pytest.mark.parametrize("tube", [True, False])
@pytest.mark.parametrize("level", [0.5, 1.5])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_small_shapes_match_the_restatement_bit_for_bit(gpu, shape, level, tube, nsteps):
    """nsteps - 1 steps of dt and a half-length last step from a smooth random l: the fp64 state, the
    last step's max |W' - W| and the fp32 table equal the restatement's exactly."""
    model = small_model(level, SHAPES[shape])
    l = smooth_target(model, seed=1)
    dt, steps, dt_last = time_step(model, horizon=(nsteps - 0.5) * _base_dt(model))
    assert steps == nsteps and dt_last < 0.75 * dt
    want, want_change = ref.solve(l, model, steps, dt, dt_last, tube)
    target = torch.from_numpy(l).to(gpu)
    table, W, change = solve_value_table(model, target, horizon=(nsteps - 0.5) * _base_dt(model), tube=tube,
                                         device=gpu, return_state=True)
    assert torch.equal(target.cpu(), torch.from_numpy(l))                 # the caller's l is not modified
    assert W.dtype == torch.float64 and tuple(W.shape) == model.shape
    assert torch.equal(W.cpu(), torch.from_numpy(want))
    assert change.item() == want_change and want_change > 0.0
    assert table.dtype == torch.float32 and tuple(table.shape) == model.shape
    assert torch.equal(table, W.to(torch.float32))
    assert torch.equal(table.cpu(), torch.from_numpy(want.astype(np.float32)))


@pytest.mark.parametrize("d", range(6))
def test_kernel_known_answer_linear_target(gpu, d):
    """l = x_d on the kernel: one tube step (and one without the min) changes l by dt min(rate, 0)
    (by dt rate) at the nodes interior along d, rate = f_d or g_d + b_d written out by hand
    (hj_solve_reference.hand_rate).  Tolerance as in tests/test_hj_solve.py: 1e-12."""
    model = small_model(1.5)
    n = model.shape
    l = np.broadcast_to(_axis(model.nodes(d), d), n).copy()
    half = 0.5 * _base_dt(model)
    dt, steps, dt_last = time_step(model, horizon=half)
    assert steps == 1
    hand = np.broadcast_to(hand_rate(model, d), n)
    interior = [slice(None)] * 6
    interior[d] = slice(1, n[d] - 1)
    interior = tuple(interior)
    for tube in (True, False):
        _, W, _ = solve_value_table(model, torch.from_numpy(l), horizon=half, tube=tube, device=gpu, return_state=True)
        got = W.cpu().numpy() - l
        want = dt_last * (np.minimum(hand, 0.0) if tube else hand)
        assert np.abs(got[interior] - want[interior]).max() < 1e-12
        assert np.abs(want[interior]).max() > 1e-7


def test_constant_target_stays_bit_constant(gpu):
    model = small_model()
    l = torch.full(model.shape, 0.37, dtype=torch.float64)
    table, W, change = solve_value_table(model, l, horizon=4.5 * _base_dt(model), device=gpu, return_state=True)
    assert torch.equal(W.cpu(), l) and change.item() == 0.0
    assert torch.equal(table.cpu(), l.to(torch.float32))


def test_level_order(gpu):
    """A stronger minimising disturbance only lowers H, so over the same horizon from the same l (the
    smooth random target of the small-shape tests) the level-0.5 table is >= the level-1.5 table at
    every node; 25 steps at level 1.5 (each level steps at its own dt).  (The order is a property of
    the PDE that the scheme keeps on a smooth l; with the kinked default target on this coarse 4 x 5
    angle grid the restatement itself breaks it at 120 nodes by up to 1e-3, so that l is not used here.)"""
    horizon = 24.5 * _base_dt(small_model(1.5))
    tables = {}
    for level in (0.5, 1.5):
        model = small_model(level)
        if level == 1.5:
            assert time_step(model, horizon)[1] == 25
        tables[level] = solve_value_table(model, torch.from_numpy(smooth_target(model, seed=0)), horizon=horizon,
                                          device=gpu)
    assert (tables[0.5] >= tables[1.5]).all()
    assert (tables[0.5] > tables[1.5]).any()


# ---- full size ----
@pytest.fixture(scope="module")
def full_model():
    return HJModel.for_config(build_config(ADV, 1), 1.5)


@pytest.fixture(scope="module")
def full_step(gpu, full_model):
    """One step at 15^6 from the default target: (l, dt_last, W') on the host, computed once."""
    half = 0.5 * _base_dt(full_model)
    dt, steps, dt_last = time_step(full_model, horizon=half)
    assert steps == 1
    l = default_target(full_model, device=gpu)
    phi, th = np.abs(_axis(full_model.nodes(0), 0)), np.abs(_axis(full_model.nodes(1), 1))
    l_host = np.ascontiguousarray(np.broadcast_to(math.pi / 2.4 - np.maximum(phi, th), full_model.shape))
    assert torch.equal(l.cpu(), torch.from_numpy(l_host))
    _, W, change = solve_value_table(full_model, l, horizon=half, device=gpu, return_state=True)
    W = W.cpu().numpy()
    assert (W <= l_host).all() and change.item() == np.abs(W - l_host).max() > 0.0     # the step moved something
    return l_host, dt_last, W


def _plane(d, k):
    axes = [np.arange(15) if a != d else np.array([k]) for a in range(6)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 6)


FULL_NODE_SETS = {
    "random_50000": lambda: np.random.default_rng(2024).integers(0, 15, size=(50000, 6)),
    "innermost_seam_lo": lambda: _plane(5, 0), "innermost_seam_hi": lambda: _plane(5, 14),
    "outermost_seam_lo": lambda: _plane(0, 0), "outermost_seam_hi": lambda: _plane(0, 14),
}


@pytest.mark.parametrize("nodes", sorted(FULL_NODE_SETS))
def test_full_size_step_matches_the_restatement(full_model, full_step, nodes):
    """15^6, level 1.5, one step: bit for bit with the indexed restatement on 50 000 seeded random
    nodes and on every node of the hyper-planes index_d in {0, 14} for d = 5 and d = 0."""
    l, dt_last, W = full_step
    idx = FULL_NODE_SETS[nodes]()
    want = ref.step_at(l, full_model, dt_last, idx, tube=True)
    got = W[tuple(idx[:, d] for d in range(6))]
    assert np.array_equal(got, want)


def test_solved_table_drives_disturbance_and_env(gpu, full_model):
    """solve_value_tables for level 1.5 at 15^6 over 20 steps.  At node-exact states the adversary
    pushes toward the nearer attitude limit: (roll +45 deg, p +0.4488) gives d0 = +dmax, (roll -55 deg,
    p -0.4488) gives d0 = -dmax, and the same pair on pitch, q gives d1 likewise; every other state
    component is zero.  (hj_disturbance returns +-dmax in every component by construction, so the
    components the state does not excite are only checked to have that magnitude.)  Then an
    adversary env bound to the table steps, and its first-step observations differ from those of the
    same env bound to an all-zero table."""
    from cf2sim.vec_env import BatchedCrazyflieEnv, hj_disturbance
    cfg = build_config(ADV, 1)
    horizon = 19.5 * _base_dt(full_model)
    assert time_step(full_model, horizon)[1] == 20
    tables = solve_value_tables(cfg, horizon=horizon, device=gpu)
    assert list(tables) == [1.5]
    table = tables[1.5]
    assert table.dtype == np.float32 and table.shape == (15,) * 6 and np.isfinite(table).all()

    ang, rate = full_model.nodes(0), full_model.nodes(3)
    assert abs(ang[12] - math.radians(45)) < 1e-12 and abs(ang[2] + math.radians(55)) < 1e-12
    assert abs(rate[8] - 0.4488) < 1e-4 and abs(rate[6] + 0.4488) < 1e-4 and abs(rate[7]) < 1e-12
    states = np.zeros((4, 6))
    states[0, 0], states[0, 3] = ang[12], rate[8]
    states[1, 0], states[1, 3] = ang[2], rate[6]
    states[2, 1], states[2, 4] = ang[12], rate[8]
    states[3, 1], states[3, 4] = ang[2], rate[6]
    _, d = hj_disturbance(torch.from_numpy(table).to(gpu), torch.from_numpy(states).to(gpu), 1.5)
    d = d.cpu().numpy()
    dmax = np.array(full_model.dmax, dtype=np.float32)
    assert d[0, 0] == dmax[0] and d[1, 0] == -dmax[0]
    assert d[2, 1] == dmax[1] and d[3, 1] == -dmax[1]
    assert np.array_equal(np.abs(d), np.broadcast_to(dmax, d.shape))

    obs = {}
    for name, tab in (("solved", table), ("zero", np.zeros_like(table))):
        env = BatchedCrazyflieEnv(ADV, 256, seed=5, device=gpu, value_tables={1.5: tab})
        env.reset()
        act = torch.zeros(256, 4, device=gpu)
        for k in range(5):
            o = env.step(act)[0]
            if k == 0:
                obs[name] = o.clone()
        env.check_device_errors()
        env.close()
    assert torch.isfinite(obs["solved"]).all()
    assert not torch.equal(obs["solved"], obs["zero"])
