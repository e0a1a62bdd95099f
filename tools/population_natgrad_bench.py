"""The TRPO / NPG update of a population against the stand-alone updaters, P members x n envs, T steps,
bf16x3 members, D = 34 (measured, not gated).

  pop        one PopulationNaturalGradientUpdater.update(rollout, read=False): every launch serves all
             P members
  separate   P NaturalGradientUpdater(fused=pop.member(m)).update(rollout.members[m], read=False) calls,
             one after the other, on the same rollouts

Settings: the defaults (10 CG iterations on every 4th row, damping 0.1, 25 line-search trials with decay
0.8, 5 x 16 value mini-batches), target_kl = 0.01.  TRPO at every shape, NPG at the first.  A member
whose line search has accepted is skipped by the later trials' launches on both sides (they return at
once), so both sides always enqueue the whole launch sequence; the accepted trials are recorded.
Per side and run: the device time of the update (device events around a window that ends in a
synchronise) and the host time until the update call(s) returned, i.e. until everything was enqueued
(time.perf_counter; where the launch queue fills, that includes waiting for the GPU).  One process,
every side warmed up once, the sides alternated inside each of --repeats runs, every run recorded.
python tools/population_natgrad_bench.py [--shapes 64x4096,8x32768,64x1024] [--steps 32]
                                         [--out profiles/population_natgrad_ab.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "disturbance-crazyfile-simulation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from population_update_bench import ENV_ID, spread, window  # noqa: E402

SETTINGS = dict(cg_iters=10, cg_damping=0.1, fvp_stride=4, line_search_steps=25, line_search_decay=0.8,
                train_v_iterations=5, num_mini_batches=16)
V_LR, TARGET_KL = 1e-3, 0.01


def launches(algorithm):
    """Kernel launches of one stand-alone update: two per gradient, evaluation or Fisher call."""
    cg, ls = SETTINGS["cg_iters"], SETTINGS["line_search_steps"]
    v = SETTINGS["train_v_iterations"] * SETTINGS["num_mini_batches"]
    policy = 2 + 2 + 1 + 3 * cg + 3 + (3 * ls if algorithm == "trpo" else 2)     # value eval, G0, cg_init, CG, direction
    return policy + 3 * v


def measure(algorithm, pop, acs, ro, repeats):
    from cf2sim.population import PopulationNaturalGradientUpdater
    from cf2sim.ppo import NaturalGradientUpdater
    P = len(pop)
    up_pop = PopulationNaturalGradientUpdater(pop, V_LR, TARGET_KL, algorithm=algorithm, **SETTINGS)
    ups = [NaturalGradientUpdater(acs[m], V_LR, TARGET_KL, algorithm=algorithm, fused=pop.member(m), **SETTINGS)
           for m in range(P)]

    def run_pop():
        up_pop.update(ro, read=False)

    def run_separate():
        for m in range(P):
            ups[m].update(ro.members[m], read=False)

    sides = {"pop": run_pop, "separate": run_separate}
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    accepted = {"pop": [r["AcceptanceStep"] for r in up_pop.result()], "separate": [u.result()["AcceptanceStep"] for u in ups]}
    dev_ms, host_ms = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            d, h = window(fn)
            dev_ms[k].append(d)
            host_ms[k].append(h)
    entry = {"kernel_launches_per_update": launches(algorithm), "warmup_acceptance_steps": accepted,
             "update": {k: spread(v) for k, v in dev_ms.items()}, "host": {k: spread(v) for k, v in host_ms.items()}}
    entry["update_separate_over_pop"] = entry["update"]["separate"]["median_ms"] / entry["update"]["pop"]["median_ms"]
    entry["host_separate_over_pop"] = entry["host"]["separate"]["median_ms"] / entry["host"]["pop"]["median_ms"]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x4096,8x32768,64x1024", help="members x envs per member")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "population_natgrad_ab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from cf2sim.population import Population, collect_population
    from cf2sim.rollout import MLPActorCritic
    from cf2sim.vec_env import BatchedCrazyflieEnv
    dev = torch.device("cuda", 0)
    T = args.steps
    result = {"device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count,
              "env": ENV_ID, "precision": "bf16x3", "obs_dim": 34, "steps": T, "repeats": args.repeats,
              "settings": {**SETTINGS, "v_lr": V_LR, "target_kl": TARGET_KL},
              "method": "device events around one update (pop) or P updates (separate), the window ending in a "
                        "synchronise; host_ms: perf_counter until the update call(s) returned; one warm-up per "
                        "side; sides alternated inside every run; every run listed", "shapes": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for i, shape in enumerate(args.shapes.split(",")):
        P, n = (int(x) for x in shape.split("x"))
        acs = []
        for m in range(P):
            torch.manual_seed(m)
            acs.append(MLPActorCritic().to(dev))
        pop = Population(acs, list(range(1, P + 1)))
        envs = BatchedCrazyflieEnv(ENV_ID, P * n, seed=1, want_final_obs=True)
        ro = collect_population(envs, pop, T)
        envs.close()
        entry = {"members": P, "envs_per_member": n, "rows_per_member": T * n}
        for algorithm in ("trpo", "npg") if i == 0 else ("trpo",):
            entry[algorithm] = measure(algorithm, pop, acs, ro, args.repeats)
        result["shapes"][shape] = entry
        print(shape, json.dumps(entry), flush=True)
        with open(args.out, "w") as f:        # after every shape: a run cut short keeps what it measured
            json.dump(result, f, indent=1)
            f.write("\n")
        del ro, pop, acs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
