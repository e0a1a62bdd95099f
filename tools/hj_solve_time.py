"""Time one full HJ value-table solve (cf2_hj_solve): the 15^6 grid of the adversary envs at
disturbance level 1.5 over the default 0.5 s horizon, from the default target.

A warm-up solve first (code objects, clocks), then --repeats timed solves, each with device events
around the whole launch sequence (the steps, the final copy when the step count is odd, the fp32
cast); the target is restored outside the timed span.  Reported per window and as the median:
ms per step, seconds per table, achieved bytes/s against the scheme's algorithmic traffic of 16 B per
node-step (one fp64 read and one fp64 write; the stencil's 12 neighbour reads are meant to hit in
cache), and that rate's fraction of the HBM peak (8.0 TB/s, the data sheet's figure).  There is no
earlier implementation to compare against and no threshold: the file is the record.

python tools/hj_solve_time.py [--level 1.5] [--horizon 0.5] [--repeats 3] [--out profiles/hj_solve.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "disturbance-crazyfile-simulation_amd"))

HBM_PEAK_BYTES_PER_S = 8.0e12
BYTES_PER_NODE_STEP = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=float, default=1.5)
    ap.add_argument("--horizon", type=float, default=0.5)
    ap.add_argument("--cfl", type=float, default=0.8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hj_solve.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hj_solve_time needs a GPU: a time taken elsewhere says nothing")
    from cf2sim import _native
    from cf2sim.config import build_config
    from cf2sim.hj_solve import DEFAULT_ENV_ID, HJModel, default_target, time_step

    dev = torch.device("cuda", 0)
    model = HJModel.for_config(build_config(DEFAULT_ENV_ID, 1), args.level)
    dt, steps, dt_last = time_step(model, args.horizon, args.cfl)
    nodes = 1
    for n in model.shape:
        nodes *= n
    l = default_target(model, device=dev)
    w, tmp = l.clone(), torch.empty_like(l)
    table = torch.empty(model.shape, dtype=torch.float32, device=dev)
    change = torch.zeros(1, dtype=torch.float64, device=dev)
    lib, m = _native.load(), model.to_c()
    stream = torch.cuda.current_stream(dev)

    def solve():
        _native.check(lib.cf2_hj_solve(ctypes.byref(m), w.data_ptr(), tmp.data_ptr(), steps, dt, dt_last, 1,
                                       table.data_ptr(), change.data_ptr(), stream.cuda_stream), "cf2_hj_solve")

    solve()                                   # warm-up
    torch.cuda.synchronize(dev)
    windows = []
    for _ in range(args.repeats):
        w.copy_(l)
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        solve()
        t1.record(stream)
        t1.synchronize()
        windows.append(t0.elapsed_time(t1) * 1e-3)
    secs = statistics.median(windows)
    rate = BYTES_PER_NODE_STEP * nodes * steps / secs
    result = {
        "what": "one cf2_hj_solve: 15^6 grid, default target, tube, fp64 state; device events around the launch sequence",
        "device": torch.cuda.get_device_name(dev), "level": args.level, "horizon_s": args.horizon, "cfl": args.cfl,
        "nodes": nodes, "dt_s": dt, "steps": steps,
        "seconds_per_table_windows": windows, "seconds_per_table": secs, "ms_per_step": secs / steps * 1e3,
        "algorithmic_bytes_per_node_step": BYTES_PER_NODE_STEP, "achieved_bytes_per_s": rate,
        "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "fraction_of_hbm_peak": rate / HBM_PEAK_BYTES_PER_S,
        "last_change": float(change.item()), "table_min": float(table.min().item()), "table_max": float(table.max().item()),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
