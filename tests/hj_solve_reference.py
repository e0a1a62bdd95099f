"""NumPy fp64 restatement of the HJ reachability scheme of csrc/cf2sim_hjsolve.hip (a helper of
tests/test_hj_solve.py and tests/test_hj_solve_gpu.py; not collected by pytest).

Every operation is written in the order the kernel's head comment states, one NumPy call per
arithmetic operation (NumPy contracts nothing), so the kernel, compiled with -ffp-contract=off, must
give the same bits.  The host-side constants are computed as cf2sim_api.cpp computes them: the same
expressions, and the C library's sin / cos / tan through Python's math module.

  coefficients(model)            inv_dx, c, b, B and the per-dimension tables
  step(W, model, dt, tube)       one step of the whole array (neighbours by np.roll)
  step_at(W, model, dt, idx, tube)   the same step at the nodes idx [K, 6] only (neighbours by flat
                                 index arithmetic: a second statement of the strides and the wrap)
  solve(l, model, steps, dt, dt_last, tube)   -> (W, max |W' - W| of the last step)
"""
import math

import numpy as np


def coefficients(model):
    n = [int(v) for v in model.n]
    I = [float(v) for v in model.inertia]
    su = 1.0 if model.u_mode == "max" else -1.0
    sd = 1.0 if model.d_mode == "max" else -1.0
    nodes = [[float(model.grid_min[d]) + float(k) * float(model.dx[d]) for k in range(n[d])] for d in range(6)]
    return {
        "n": n,
        "periodic": [bool((int(model.periodic_mask) >> d) & 1) for d in range(6)],
        "inv_dx": [1.0 / float(model.dx[d]) for d in range(6)],
        "c": [(I[1] - I[2]) / I[0], (I[2] - I[0]) / I[1], (I[0] - I[1]) / I[2]],
        "b": [(su * float(model.umax[k]) + sd * float(model.dmax[k])) / I[k] for k in range(3)],
        "B": [(float(model.umax[k]) + float(model.dmax[k])) / I[k] for k in range(3)],
        "nodes": [np.array(v, dtype=np.float64) for v in nodes],
        "sin_phi": np.array([math.sin(v) for v in nodes[0]], dtype=np.float64),
        "cos_phi": np.array([math.cos(v) for v in nodes[0]], dtype=np.float64),
        "tan_theta": np.array([math.tan(v) for v in nodes[1]], dtype=np.float64),
        "sec_theta": np.array([1.0 / math.cos(v) for v in nodes[1]], dtype=np.float64),
    }


def drift(co, sphi, cphi, tth, scth, p, q, r):
    """f0..f2 and the gyroscopic terms g3..g5 (arrays that broadcast against each other)."""
    mix = q * sphi + r * cphi
    f = [p + mix * tth, q * cphi - r * sphi, mix * scth]
    g = [co["c"][0] * (q * r), co["c"][1] * (p * r), co["c"][2] * (p * q)]
    return f, g


def _update(co, W, Wm, Wp, at_lo, at_hi, f, g, dt, tube):
    """W' from W, its neighbours Wm[d] / Wp[d] (any value where a non-periodic boundary has none:
    at_lo[d] / at_hi[d] mark those nodes), the drift f and the gyroscopic terms g."""
    sg = np.sign(W)
    a, e = [], []
    for d in range(6):
        wm, wp = Wm[d], Wp[d]
        if not co["periodic"][d]:
            wm = np.where(at_lo[d], W + np.abs(wp - W) * sg, wm)
            wp = np.where(at_hi[d], W + np.abs(W - wm) * sg, wp)
        dm = (W - wm) * co["inv_dx"][d]
        dp = (wp - W) * co["inv_dx"][d]
        a.append(0.5 * (dm + dp))
        e.append(0.5 * (dp - dm))
    H = np.zeros_like(W)
    for d in range(3):
        H = H + f[d] * a[d]
        H = H + np.abs(f[d]) * e[d]
    for d in range(3, 6):
        k = d - 3
        H = H + g[k] * a[d]
        H = H + co["b"][k] * np.abs(a[d])
        H = H + (np.abs(g[k]) + co["B"][k]) * e[d]
    rate = np.where(H < 0.0, H, 0.0) if tube else H
    return W + dt * rate


def _axis(v, d):
    shape = [1] * 6
    shape[d] = -1
    return np.asarray(v).reshape(shape)


def step(W, model, dt, tube=True, co=None):
    co = co or coefficients(model)
    n = co["n"]
    assert W.dtype == np.float64 and list(W.shape) == n
    Wm = [np.roll(W, 1, axis=d) for d in range(6)]
    Wp = [np.roll(W, -1, axis=d) for d in range(6)]
    at_lo = [_axis(np.arange(n[d]) == 0, d) for d in range(6)]
    at_hi = [_axis(np.arange(n[d]) == n[d] - 1, d) for d in range(6)]
    f, g = drift(co, _axis(co["sin_phi"], 0), _axis(co["cos_phi"], 0), _axis(co["tan_theta"], 1),
                 _axis(co["sec_theta"], 1), _axis(co["nodes"][3], 3), _axis(co["nodes"][4], 4), _axis(co["nodes"][5], 5))
    return _update(co, W, Wm, Wp, at_lo, at_hi, f, g, dt, tube)


def step_at(W, model, dt, idx, tube=True, co=None):
    """W' at the nodes idx [K, 6] (per-dimension indices), as a [K] array."""
    co = co or coefficients(model)
    n = co["n"]
    flat = np.ascontiguousarray(W).reshape(-1)
    idx = np.asarray(idx, dtype=np.int64)
    stride = [int(np.prod(n[d + 1:], dtype=np.int64)) for d in range(6)]
    c = sum(idx[:, d] * stride[d] for d in range(6))
    Wm, Wp, at_lo, at_hi = [], [], [], []
    for d in range(6):
        lo, hi = idx[:, d] == 0, idx[:, d] == n[d] - 1
        # the far end on a periodic dimension; the node itself where there is no neighbour
        far = (n[d] - 1) * stride[d] if co["periodic"][d] else 0
        Wm.append(flat[np.where(lo, c + far, c - stride[d])])
        Wp.append(flat[np.where(hi, c - far, c + stride[d])])
        at_lo.append(lo)
        at_hi.append(hi)
    f, g = drift(co, co["sin_phi"][idx[:, 0]], co["cos_phi"][idx[:, 0]], co["tan_theta"][idx[:, 1]],
                 co["sec_theta"][idx[:, 1]], co["nodes"][3][idx[:, 3]], co["nodes"][4][idx[:, 4]],
                 co["nodes"][5][idx[:, 5]])
    return _update(co, flat[c], Wm, Wp, at_lo, at_hi, f, g, dt, tube)


def solve(l, model, steps, dt, dt_last, tube=True, history=None):
    """(W after steps - 1 steps of dt and one of dt_last, max |W' - W| of the last step); with a
    list as ``history`` every intermediate W is appended to it."""
    co = coefficients(model)
    W = np.array(l, dtype=np.float64)
    change = 0.0
    for k in range(steps):
        Wn = step(W, model, dt_last if k == steps - 1 else dt, tube, co)
        change = float(np.max(np.abs(Wn - W)))
        W = Wn
        if history is not None:
            history.append(W)
    return W, change


# ---- shared inputs of the two test files (nothing below is used by the restatement above) ----
ADV = "DroneHoverBulletFreeEnvWithAdversary-v0"
SHAPE = (4, 5, 6, 3, 7, 8)               # 20 160 nodes: no multiple of the kernel's 256-thread blocks


def small_model(level=1.5, shape=SHAPE, **kw):
    """The adversary env's constants on a small mixed shape over the full grid's ranges."""
    from cf2sim.config import build_config
    from cf2sim.hj_solve import HJModel
    full = HJModel.for_config(build_config(ADV, 1), level, **kw)
    lo = [-math.pi / 2.4] * 3 + [-math.pi] * 3
    hi = [math.pi / 2.4] * 3 + [math.pi] * 3
    dx = [(hi[d] - lo[d]) / (shape[d] if d < 3 else shape[d] - 1) for d in range(6)]   # periodic: upper end excluded
    return HJModel(n=shape, grid_min=tuple(lo), dx=tuple(dx), periodic_mask=0b000111, inertia=full.inertia,
                   umax=full.umax, dmax=full.dmax, u_mode=full.u_mode, d_mode=full.d_mode)


def smooth_target(model, seed=0):
    """A smooth random l: a few random low-frequency products, periodic along the angle dims."""
    rng = np.random.default_rng(seed)
    n = model.shape
    l = np.zeros(n)
    for _ in range(4):
        term = np.ones(n)
        for d in range(6):
            u = np.arange(n[d]) / (n[d] if d < 3 else n[d] - 1)
            k = 1.0 if d < 3 else rng.uniform(0.3, 1.2)
            term = term * _axis(1.0 + 0.5 * np.sin(2.0 * np.pi * k * u + rng.uniform(0, 2 * np.pi)), d)
        l = l + rng.uniform(-1.0, 1.0) * term
    return l


def hand_rate(model, d):
    """f_d (d < 3) or g_d + b_d (d >= 3) at every node, written out from the model's equations with
    NumPy's own sin / cos / tan and none of the restatement's code: with l = x_d, grad l = e_d, so
    one step changes l by dt min(hand_rate, 0) (tube) or dt hand_rate at the nodes interior along d."""
    x = [np.array(model.nodes(k)) for k in range(6)]
    phi, th = _axis(x[0], 0), _axis(x[1], 1)
    p, q, r = _axis(x[3], 3), _axis(x[4], 4), _axis(x[5], 5)
    Ixx, Iyy, Izz = model.inertia
    su, sd = (1 if model.u_mode == "max" else -1), (1 if model.d_mode == "max" else -1)
    return [p + (q * np.sin(phi) + r * np.cos(phi)) * np.tan(th),
            q * np.cos(phi) - r * np.sin(phi),
            (q * np.sin(phi) + r * np.cos(phi)) / np.cos(th),
            (Iyy - Izz) / Ixx * q * r + (su * model.umax[0] + sd * model.dmax[0]) / Ixx,
            (Izz - Ixx) / Iyy * p * r + (su * model.umax[1] + sd * model.dmax[1]) / Iyy,
            (Ixx - Iyy) / Izz * p * q + (su * model.umax[2] + sd * model.dmax[2]) / Izz][d]


def alpha_sum(model):
    """sum_d alpha_d(x) / dx_d at every node (the time step's bound), by brute force over the whole grid."""
    co = coefficients(model)
    f, g = drift(co, _axis(co["sin_phi"], 0), _axis(co["cos_phi"], 0), _axis(co["tan_theta"], 1),
                 _axis(co["sec_theta"], 1), _axis(co["nodes"][3], 3), _axis(co["nodes"][4], 4), _axis(co["nodes"][5], 5))
    total = np.zeros(co["n"], dtype=np.float64)
    for d in range(3):
        total = total + np.abs(f[d]) * co["inv_dx"][d]
    for d in range(3, 6):
        total = total + (np.abs(g[d - 3]) + co["B"][d - 3]) * co["inv_dx"][d]
    return total
