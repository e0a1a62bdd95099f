"""HJ value tables: solve the reachability PDE on the GPU (cf2_hj_solve, csrc/cf2sim_hjsolve.hip).

The HJ-adversary envs read one 15^6 value table per disturbance level.  The reference's tables are
large files outside its repository, made by a solver that is not part of it; this module produces
tables with this project's own model and scheme (include/cf2sim.h, cf2_hj_model), built from the
project's own constants.  **Parity with the reference's own tables is unpinned**: nothing here was
compared against them.  Tables supplied by the user (``value_tables=``) keep working unchanged.

    tables = solve_value_tables(cfg)                      # {level: float32 [15]*6}
    env = BatchedCrazyflieEnv(env_id, n, value_tables=tables)
    save_value_tables("tables/", tables)                  # fastrack_{level}_15x15.npy, as the reference names them

    python -m cf2sim.hj_solve --levels 0.0:3.0:0.1 --out DIR [--horizon S]

State x = [roll, pitch, yaw, p, q, r] (the table's C-order axes).  W(x, tau) advances from the target
function W(x, 0) = l(x) by W_tau = min(0, H) (a backward reachable tube; ``tube=False``: W_tau = H),
H = opt_u opt_d grad W . f.  The step kernel applies the disturbance that decreases V fastest, so by
default the disturbance minimises and the control maximises.
"""
from __future__ import annotations

import ctypes
import math
import os
import time
from dataclasses import dataclass

import numpy as np

ANGLE_LIMIT = math.pi / 2.4          # the adversary envs' 75 degree done threshold
DEFAULT_ENV_ID = "DroneHoverBulletFreeEnvWithAdversary-v0"


@dataclass
class HJModel:
    """Mirror of cf2_hj_model: grid, inertia diagonal, input bounds and the players' roles."""
    n: tuple = (15,) * 6
    grid_min: tuple = (0.0,) * 6
    dx: tuple = (1.0,) * 6
    periodic_mask: int = 0b000111           # bit d: dimension d wraps (upper end excluded)
    inertia: tuple = (1.0, 1.0, 1.0)
    umax: tuple = (0.0, 0.0, 0.0)
    dmax: tuple = (0.0, 0.0, 0.0)
    u_mode: str = "max"
    d_mode: str = "min"

    def __post_init__(self):
        for name in ("u_mode", "d_mode"):
            if getattr(self, name) not in ("min", "max"):
                raise ValueError(f"{name} must be 'min' or 'max'")

    @classmethod
    def for_config(cls, cfg, level: float, inertia=None, u_mode: str = "max", d_mode: str = "min") -> "HJModel":
        """The model of an env configuration at a disturbance level: cfg's HJ grid (config.hj_grid),
        its disturbance bound (cfg.dstb_umax) as the control bound, level times it as the disturbance
        bound, and the inertia diagonal the config read from the URDF (or ``inertia``)."""
        from .config import HJ_PTS
        umax = tuple(float(cfg.dstb_umax[k]) for k in range(3))
        inertia = (float(cfg.ixx), float(cfg.iyy), float(cfg.izz)) if inertia is None else tuple(float(v) for v in inertia)
        return cls(n=(HJ_PTS,) * 6, grid_min=tuple(float(cfg.hj_grid_min[d]) for d in range(6)),
                   dx=tuple(float(cfg.hj_grid_dx[d]) for d in range(6)), periodic_mask=0b000111, inertia=inertia,
                   umax=umax, dmax=tuple(float(level) * u for u in umax), u_mode=u_mode, d_mode=d_mode)

    @property
    def shape(self) -> tuple:
        return tuple(int(v) for v in self.n)

    def nodes(self, d: int) -> list:
        """Node values of dimension d, grid_min + k dx, as the library computes them."""
        return [self.grid_min[d] + float(k) * self.dx[d] for k in range(int(self.n[d]))]

    def to_c(self):
        from ._native import CF2HJModel
        m = CF2HJModel()
        for d in range(6):
            m.n[d], m.grid_min[d], m.dx[d] = int(self.n[d]), float(self.grid_min[d]), float(self.dx[d])
        for k in range(3):
            m.inertia[k], m.umax[k], m.dmax[k] = float(self.inertia[k]), float(self.umax[k]), float(self.dmax[k])
        m.periodic_mask = int(self.periodic_mask)
        m.u_max_player, m.d_max_player = int(self.u_mode == "max"), int(self.d_mode == "max")
        return m


def _device(device):
    import torch
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def default_target(model: HJModel, angle_limit: float = ANGLE_LIMIT, device=None):
    """l(x) = angle_limit - max(|roll|, |pitch|), the margin to the adversary envs' done threshold,
    as an fp64 device tensor of the model's shape."""
    import torch
    dev = _device(device)
    phi = torch.tensor(model.nodes(0), dtype=torch.float64, device=dev).abs().reshape(-1, 1, 1, 1, 1, 1)
    theta = torch.tensor(model.nodes(1), dtype=torch.float64, device=dev).abs().reshape(1, -1, 1, 1, 1, 1)
    return (float(angle_limit) - torch.maximum(phi, theta)).expand(model.shape).contiguous()


def time_step(model: HJModel, horizon: float = 0.5, cfl: float = 0.8) -> tuple:
    """(dt, steps, dt_last): dt = cfl / max_x sum_d alpha_d(x) / dx_d (cf2_hj_time_step, on the host),
    the number of steps that covers ``horizon`` and the shortened last step that lands on it."""
    from . import _native
    if not horizon > 0.0:
        raise ValueError("horizon must be positive")
    dt = ctypes.c_double()
    m = model.to_c()
    _native.check(_native.load().cf2_hj_time_step(ctypes.byref(m), float(cfl), ctypes.byref(dt)), "cf2_hj_time_step")
    dt = dt.value
    steps = max(1, math.ceil(horizon / dt - 1e-9))
    dt_last = horizon - (steps - 1) * dt
    return dt, steps, dt_last


def solve_value_table(model: HJModel, target=None, horizon: float = 0.5, cfl: float = 0.8, tube: bool = True,
                      device=None, return_state: bool = False):
    """The value table of ``model``: a float32 device tensor of the model's shape.  ``target``: l(x),
    an fp64 tensor of that shape (default: ``default_target``); it is not modified.  The default
    horizon is about the time the top grid rate (pi rad/s) takes to cross the 75 degree range.
    The solve is a fixed sequence of launches on the current stream; the host reads nothing between
    them.  With ``return_state`` also the fp64 W and the last step's max |W' - W| (a one-element
    device tensor)."""
    import torch
    from . import _native
    dev = _device(device)
    dt, steps, dt_last = time_step(model, horizon, cfl)
    if target is None:
        w = default_target(model, device=dev)
    else:
        if tuple(target.shape) != model.shape:
            raise ValueError(f"target must have the model's shape {model.shape}")
        w = target.to(device=dev, dtype=torch.float64).contiguous().clone()
    tmp = torch.empty_like(w)
    table = torch.empty(model.shape, dtype=torch.float32, device=dev)
    change = torch.zeros(1, dtype=torch.float64, device=dev)
    m = model.to_c()
    with torch.cuda.device(dev):
        _native.check(_native.load().cf2_hj_solve(ctypes.byref(m), w.data_ptr(), tmp.data_ptr(), steps, dt, dt_last,
                                                  int(bool(tube)), table.data_ptr(), change.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "cf2_hj_solve")
    if return_state:
        return table, w, change
    return table


def _levels_of(cfg_or_levels):
    from .config import CF2Config, build_config
    if isinstance(cfg_or_levels, CF2Config):
        cfg = cfg_or_levels
        if int(cfg.level_mode) == 1:        # Boltzmann level per episode: one table per level
            return cfg, [float(cfg.level_values[k]) for k in range(int(cfg.num_levels))]
        return cfg, [float(cfg.dstb_level)]
    levels = [float(cfg_or_levels)] if isinstance(cfg_or_levels, (int, float)) else [float(v) for v in cfg_or_levels]
    return build_config(DEFAULT_ENV_ID, 1), levels


def solve_value_tables(cfg_or_levels, target=None, horizon: float = 0.5, cfl: float = 0.8, tube: bool = True,
                       device=None, inertia=None, report=None) -> dict:
    """{level: float32 numpy [15]*6} for an env configuration (its level, or every level of
    ``cfg.level_values`` for a Boltzmann-level config) or for a list of levels (on the default
    adversary env's grid and constants); usable directly as ``BatchedCrazyflieEnv(..., value_tables=...)``.
    ``report(level, steps, last_change, seconds)`` is called per table."""
    import torch
    cfg, levels = _levels_of(cfg_or_levels)
    dev = _device(device)
    tables = {}
    for lv in levels:
        model = HJModel.for_config(cfg, lv, inertia=inertia)
        t0 = time.perf_counter()
        table, _, change = solve_value_table(model, target, horizon, cfl, tube, dev, return_state=True)
        tables[lv] = table.cpu().numpy()          # the copy waits for the solve
        if report is not None:
            report(lv, time_step(model, horizon, cfl)[1], float(change.item()), time.perf_counter() - t0)
        del table
    torch.cuda.synchronize(dev)
    return tables


def save_value_tables(directory, tables: dict) -> list:
    """Write each table as ``value_table_name(level)`` (the reference's file names) into
    ``directory``; ``load_value_tables(directory, cfg)`` / ``value_tables=directory`` read them back."""
    from .vec_env import value_table_name
    os.makedirs(directory, exist_ok=True)
    paths = []
    for lv, table in tables.items():
        path = os.path.join(os.fspath(directory), value_table_name(lv))
        np.save(path, np.asarray(table, dtype=np.float32))
        paths.append(path)
    return paths


def parse_levels(text: str) -> list:
    """'1.5', '0.5,1.5' or 'start:stop:step' (stop included), rounded to one decimal like the
    reference's file names."""
    if ":" in text:
        lo, hi, step = (float(v) for v in text.split(":"))
        if not step > 0.0:
            raise ValueError("the level step must be positive")
        return [round(lo + k * step, 1) for k in range(int(math.floor((hi - lo) / step + 1e-9)) + 1)]
    return [round(float(v), 1) for v in text.split(",")]


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m cf2sim.hj_solve", description=(
        "Solve the HJ value tables of the adversary hover envs on the GPU and write them under the reference's "
        "file names.  The model and scheme are this project's own: parity with the reference's tables is unpinned."))
    ap.add_argument("--levels", required=True, help="'1.5', '0.5,1.5' or 'start:stop:step' (stop included)")
    ap.add_argument("--out", required=True, help="directory for the fastrack_{level}_15x15.npy files")
    ap.add_argument("--horizon", type=float, default=0.5, help="seconds of reachability horizon (default 0.5)")
    ap.add_argument("--cfl", type=float, default=0.8)
    args = ap.parse_args(argv)

    def report(level, steps, change, seconds):
        print(f"level {level}: {steps} steps, last change {change:.3e}, {seconds:.2f} s", flush=True)

    for lv in parse_levels(args.levels):     # one table in host memory at a time
        save_value_tables(args.out, solve_value_tables([lv], horizon=args.horizon, cfl=args.cfl, report=report))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
