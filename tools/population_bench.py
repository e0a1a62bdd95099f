"""Populations against the stand-alone paths, P members x n envs, bf16x3, D = 34 (measured, not gated).

Forward, one call on [P * n, D] observations:
  pop        one cf2_policy_forward_pop launch
  separate   P cf2_policy_forward launches, one per member's rows
  single     one cf2_policy_forward launch over all P * n rows (one weight set: the kernel's floor)
Collect, T env-steps of every env, time per population env-step (all P * n envs stepped once):
  pop        collect_population on one context of P * n envs, its member-major copy included
  separate   the sum of P collect(..., fuse=True) calls on contexts of n envs (env_id_offset = m * n)
  copy       collect_population's member-major copy alone

One process, device events around each window (a window ends in a synchronise), every side warmed
up, the sides alternated inside each of --repeats runs, every run recorded.
python tools/population_bench.py [--shapes 64x4096,8x32768] [--steps 32] [--out profiles/population_ab.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "disturbance-crazyfile-simulation_amd"))

ENV_ID = "DroneHoverBulletFreeEnvWithGust-v0"


def window_us(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def spread(v, inner):
    return {"runs_us": v, "min_us": min(v), "median_us": statistics.median(v), "max_us": max(v), "calls_per_window": inner}


def measure(sides, repeats, warmup):
    for fn, _ in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(repeats):
        for k, (fn, inner) in sides.items():
            times[k].append(window_us(fn, inner))
    return {k: spread(v, sides[k][1]) for k, v in times.items()}


def learners(P, dev):
    from cf2sim.rollout import MLPActorCritic
    acs = []
    for m in range(P):
        torch.manual_seed(m)
        acs.append(MLPActorCritic().to(dev))
    return acs


def forward_sides(pop, solos, P, n, dev, inner):
    from cf2sim import _native
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    d = pop.obs_dim
    obs = torch.randn(P * n, d, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    act, val, logp = torch.empty(P * n, 4, device=dev), torch.empty(P * n, device=dev), torch.empty(P * n, device=dev)
    o_p, a_p, v_p, l_p = obs.data_ptr(), act.data_ptr(), val.data_ptr(), logp.data_ptr()

    def run_pop():
        pop.step_into(obs, act, val, logp)

    def run_separate():
        for m, f in enumerate(solos):
            r = m * n
            _native.check(lib.cf2_policy_forward(f.w_ptr, n, d, f.prec, o_p + r * d * 4, f.seed, f.counter & 0xFFFFFFFF, r,
                                                 1, a_p + r * 16, v_p + r * 4, l_p + r * 4, stream), "cf2_policy_forward")
            f.counter += 1

    def run_single():
        solos[0].step_into(obs, act, val, logp)

    return {"pop": (run_pop, inner), "separate": (run_separate, inner), "single": (run_single, inner)}


def collect_sides(pop, solos, P, n, T, dev, inner):
    from cf2sim.population import _MOVED, collect_population, member_major
    from cf2sim.rollout import collect
    from cf2sim.vec_env import BatchedCrazyflieEnv
    big = BatchedCrazyflieEnv(ENV_ID, P * n, seed=1, want_final_obs=True)
    small = [BatchedCrazyflieEnv(ENV_ID, n, seed=1, env_id_offset=m * n, want_final_obs=True) for m in range(P)]
    state = {"pop": collect_population(big, pop, T), "solo": [collect(e, f, T, fuse=True) for e, f in zip(small, solos)]}
    assert all(e.last_collect_fused is True for e in small), "the stand-alone collects did not run in one launch"

    def run_pop():
        state["pop"] = collect_population(big, pop, T, obs=state["pop"].last_obs, out=state["pop"])

    def run_separate():
        for m in range(P):
            ro = state["solo"][m]
            state["solo"][m] = collect(small[m], solos[m], T, obs=ro.last_obs, fuse=True, out=ro)

    def run_copy():
        S = state["pop"].storage
        for name, extra in _MOVED:
            member_major(S["loop"][name][:T + extra], P, out=S["member"][name])

    return {"pop": (run_pop, inner), "separate": (run_separate, inner), "copy": (run_copy, inner)}, [big] + small


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x4096,8x32768", help="members x envs per member")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inner-forward", type=int, default=200)
    ap.add_argument("--inner-collect", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "population_ab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from cf2sim import _native
    from cf2sim.population import Population
    from cf2sim.rollout import FusedActorCritic
    dev = torch.device("cuda", 0)
    T = args.steps
    result = {"device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count,
              "env": ENV_ID, "precision": "bf16x3", "obs_dim": 34, "steps": T, "repeats": args.repeats,
              "method": "device events around windows ending in a synchronise; 3 warm-up calls per side; sides "
                        "alternated inside every run; every run listed (runs_us, per call)", "shapes": {}}
    for shape in args.shapes.split(","):
        P, n = (int(x) for x in shape.split("x"))
        acs = learners(P, dev)
        pop = Population(acs, list(range(1, P + 1)))
        solos = [FusedActorCritic(ac, seed=m + 1) for m, ac in enumerate(acs)]
        entry = {"members": P, "envs_per_member": n, "blocks_per_member": int(_native.load().cf2_policy_pop_blocks(P, n))}
        fwd = measure(forward_sides(pop, solos, P, n, dev, args.inner_forward), args.repeats, 3)
        entry["forward"] = fwd
        entry["forward_separate_over_pop"] = fwd["separate"]["median_us"] / fwd["pop"]["median_us"]
        entry["forward_pop_over_single"] = fwd["pop"]["median_us"] / fwd["single"]["median_us"]
        sides, envs = collect_sides(pop, solos, P, n, T, dev, args.inner_collect)
        col = measure(sides, args.repeats, 3)
        for v in col.values():
            v["median_us_per_env_step"] = v["median_us"] / T
        entry["collect"] = col
        entry["collect_separate_over_pop"] = col["separate"]["median_us"] / col["pop"]["median_us"]
        entry["collect_copy_share_of_pop"] = col["copy"]["median_us"] / col["pop"]["median_us"]
        for e in envs:
            e.close()
        result["shapes"][shape] = entry
        print(shape, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
