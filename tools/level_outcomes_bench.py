"""Time cf2_level_outcomes beside cf2_episode_stats on the same [T, N] buffers, and the fused collect
(cf2_collect_rollout) with and without its cost / level outputs, in one process with the sides
alternated (device events after a warm-up; min / median / max over --repeats windows).
The scan inputs rotate over enough buffer sets to exceed the 256 MiB cache.  Measured, not gated.
python tools/level_outcomes_bench.py [--envs 32768,262144] [--steps 32] [--levels 21] [--out profiles/level_outcomes.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "disturbance-crazyfile-simulation_amd"))


def window_us(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(inner):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def spread(v):
    return {"min_us": min(v), "median_us": statistics.median(v), "max_us": max(v), "windows": len(v)}


def scan_sides(lib, _native, T, n, L, dev, done_rate):
    from cf2sim.config import boltzmann_table
    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(0)
    rows = T * n
    nsets = max(2, -(-(320 << 20) // (rows * 14)))
    lv = torch.tensor(boltzmann_table()[0][:L] if L <= 21 else [0.125 * k for k in range(L)], dtype=torch.float32, device=dev)
    sets = []
    for _ in range(nsets):
        done = (torch.rand(T, n, device=dev, generator=g) < done_rate).to(torch.uint8)
        sets.append(dict(rew=torch.randn(T, n, device=dev, generator=g), cost=torch.rand(T, n, device=dev, generator=g),
                         done=done, trunc=done * (torch.rand(T, n, device=dev, generator=g) < 0.5).to(torch.uint8),
                         level=lv[torch.randint(0, L, (T, n), device=dev, generator=g)].contiguous()))
    cr, cc = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    cl = torch.zeros(n, dtype=torch.int32, device=dev)
    summary = torch.zeros(16, dtype=torch.float64, device=dev)
    escratch = torch.empty(lib.cf2_episode_stats_scratch_bytes(n) // 8, dtype=torch.float64, device=dev)
    table = torch.zeros(L + 1, 16, dtype=torch.float64, device=dev)
    oscratch = torch.empty(lib.cf2_level_outcomes_scratch_bytes(T, n, L) // 8 + 1, dtype=torch.float64, device=dev)

    def episode_stats(i):
        s = sets[i % nsets]
        _native.check(lib.cf2_episode_stats(T, n, s["rew"].data_ptr(), s["cost"].data_ptr(), s["done"].data_ptr(),
                                            cr.data_ptr(), cc.data_ptr(), cl.data_ptr(), None, None, None,
                                            summary.data_ptr(), 1, escratch.data_ptr(), stream), "cf2_episode_stats")

    def level_outcomes(i):
        s = sets[i % nsets]
        _native.check(lib.cf2_level_outcomes(T, n, s["rew"].data_ptr(), s["cost"].data_ptr(), s["done"].data_ptr(),
                                             s["trunc"].data_ptr(), s["level"].data_ptr(), lv.data_ptr(), L, cr.data_ptr(),
                                             cc.data_ptr(), cl.data_ptr(), None, table.data_ptr(), 1, oscratch.data_ptr(),
                                             stream), "cf2_level_outcomes")

    read = rows * 14 + n * 24                     # rew, cost, level, done, trunc; carries read and written
    records = rows * 2 + int(rows * done_rate) * 24       # tags written and read once; records written and read
    return ({"episode_stats_cost": episode_stats, "level_outcomes": level_outcomes},
            {"buffer_sets": nsets, "episode_stats_bytes": rows * 9 + n * 24, "level_outcomes_read_bytes": read,
             "level_outcomes_record_bytes": records, "done_rate": done_rate})


def collect_sides(n, T, dev):
    from cf2sim.rollout import FusedActorCritic, MLPActorCritic
    from cf2sim.vec_env import BatchedCrazyflieEnv
    envs = BatchedCrazyflieEnv("DroneHoverBulletFreeEnvWithGust-v0", n, seed=1, want_final_obs=True)
    torch.manual_seed(0)
    ac = FusedActorCritic(MLPActorCritic(obs_dim=envs.obs_dim).to(dev), seed=3)
    d = envs.obs_dim
    e = lambda *shape, dt=torch.float32: torch.empty(*shape, device=dev, dtype=dt)
    obs, fin, act, val, logp = e(T + 1, n, d), e(T, n, d), e(T + 1, n, 4), e(T + 1, n), e(T + 1, n)
    rew, cost, level, d8, tr8 = e(T, n), e(T, n), e(T, n), e(T, n, dt=torch.uint8), e(T, n, dt=torch.uint8)
    obs[0].copy_(envs.reset())
    ac.step_into(obs[0], act[0], val[0], logp[0])

    def run(info):
        def call(_):
            ok = envs.collect_rollout_into(act, obs[1:], rew, d8, tr8, fin, ac, val, logp,
                                           **({"cost_out": cost, "level_out": level} if info else {}))
            assert ok, "no fused collect instance for this configuration"
            act[0].copy_(act[T])                  # the next call continues from the last sampled actions
        return call
    return {"collect_rollout": run(False), "collect_rollout_info": run(True)}, envs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="32768,262144")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--levels", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--done-rate", type=float, default=0.002, help="episode ends per slot (1 / 500 steps)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_outcomes.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from cf2sim import _native
    lib = _native.load()
    dev = torch.device("cuda", 0)
    T, L = args.steps, args.levels
    result = {"device": torch.cuda.get_device_name(0), "steps": T, "levels": L, "repeats": args.repeats,
              "method": "device events, sides alternated inside every repeat, 3 warm-up calls per side", "sizes": {}}
    for n in [int(x) for x in args.envs.split(",")]:
        scan, meta = scan_sides(lib, _native, T, n, L, dev, args.done_rate)
        coll, envs = collect_sides(n, T, dev)
        sides = {k: (f, args.inner) for k, f in scan.items()}
        sides.update({k: (f, max(2, args.inner // 10)) for k, f in coll.items()})
        for fn, _ in sides.values():
            for i in range(3):
                fn(i)
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, (fn, inner) in sides.items():
                times[k].append(window_us(fn, inner))
        entry = dict(meta)
        for k, v in times.items():
            entry[k] = spread(v)
            entry[k]["calls_per_window"] = sides[k][1]
        for k in ("collect_rollout", "collect_rollout_info"):
            entry[k]["median_us_per_env_step"] = entry[k]["median_us"] / T
        lo = entry["level_outcomes"]["median_us"]
        entry["level_outcomes_read_TBps"] = meta["level_outcomes_read_bytes"] / lo * 1e-6
        entry["level_outcomes_total_TBps"] = (meta["level_outcomes_read_bytes"] + meta["level_outcomes_record_bytes"]) / lo * 1e-6
        entry["episode_stats_TBps"] = meta["episode_stats_bytes"] / entry["episode_stats_cost"]["median_us"] * 1e-6
        result["sizes"][str(n)] = entry
        envs.close()
        print(n, json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
