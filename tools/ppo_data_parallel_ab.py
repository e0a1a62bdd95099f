"""A/B of the second merge level of the data-parallel PPO update, in one process with the sides
alternated (one warm-up window and --repeats windows per side; min / median / max):

    single    ResidentPPOUpdater(group=None): the launch sequence of a single rank, as before the
              rank-partial calls existed (compare with resident_wall of profiles/ppo_resident_ab.json,
              same shape and settings)
    partial   ResidentPPOUpdater(group=RankReducer(None, force=True)): every gradient and evaluation
              call as rank partial -> reduce over one block, the advantage moments as
              cf2_column_moments_partial -> cf2_moments_combine: the cost of the extra merge level with
              no link in it

A window is one ``update(rollout, read=False)`` plus the final device read (``result()``), on the host
clock; the same synthetic rollout and starting weights for both sides (reloaded before every window,
outside the timed span).

What this does not measure: a process group.  Two gloo ranks stage every all-gather through the host
and are a rehearsal path, not a performance figure; RCCL at world > 1 needs more than one GPU.  Per
gathered block a rank sends cf2_ppo_partial_doubles(obs_dim) doubles (51 784 bytes at obs_dim 34).

python tools/ppo_data_parallel_ab.py [--envs 32768] [--steps 32] [--out profiles/ppo_data_parallel_ab.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "disturbance-crazyfile-simulation_amd"))


def stats(v):
    return {"min_ms": min(v), "median_ms": statistics.median(v), "max_ms": max(v)}


def measure(envs, args, dev):
    from cf2sim.dist import RankReducer
    from cf2sim.ppo import ResidentPPOUpdater
    from cf2sim.rollout import MLPActorCritic, Rollout
    T, d = args.steps, args.obs_dim
    g = torch.Generator(device=dev).manual_seed(0)
    torch.manual_seed(0)
    ac = MLPActorCritic(obs_dim=d).to(dev)
    obs = torch.randn(T, envs, d, device=dev, generator=g)
    with torch.no_grad():
        act, val, logp = ac.step(obs.view(-1, d), generator=g)
    adv = torch.randn(T, envs, device=dev, generator=g)
    ret = torch.randn(T, envs, device=dev, generator=g)
    z = torch.zeros(1, device=dev)
    ro = Rollout(obs, act.view(T, envs, 4), z, val.view(T, envs), logp.view(T, envs), z.bool(), z.bool(), adv, ret, obs[0],
                 z, z, z)
    start = copy.deepcopy(ac.state_dict())
    kw = dict(train_pi_iterations=args.pi_iters, train_v_iterations=args.v_iters, num_mini_batches=16)
    mk = lambda group: ResidentPPOUpdater(ac, 3e-4, 1e-3, 0.2, 1e9, generator=torch.Generator(device=dev).manual_seed(1),
                                          group=group, **kw)
    ups = {"single": mk(None), "partial": mk(RankReducer(None, force=True))}

    def window(side):
        ac.load_state_dict(start)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ups[side].update(ro, read=False)
        out = ups[side].result()
        return (time.perf_counter() - t0) * 1e3, out

    last, times = {}, {s: [] for s in ups}
    for s in ups:                         # warm up every path
        _, last[s] = window(s)
    for _ in range(args.repeats):         # the sides alternate inside every repeat
        for s in ups:
            t, last[s] = window(s)
            times[s].append(t)
    res = {s + "_wall": stats(v) for s, v in times.items()}
    same = all(last["single"][k] == last["partial"][k] for k in last["single"])
    return {"envs": envs, "steps": T, "rows": T * envs, "sides": res,
            "partial_over_single_wall": res["partial_wall"]["median_ms"] / res["single_wall"]["median_ms"],
            "same_result_bits": same, "last_update": last}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--obs-dim", type=int, default=34)
    ap.add_argument("--pi-iters", type=int, default=80)
    ap.add_argument("--v-iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_data_parallel_ab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "obs_dim": args.obs_dim, "pi_iterations": args.pi_iters,
           "v_iterations": args.v_iters, "mini_batches": 16, "target_kl": 1e9, "repeats": args.repeats,
           "timing": "host clock around one update(read=False) plus the final device read; one warm-up window per side, "
                     "sides alternated; single: group=None; partial: a world-1 reducer forced through partial -> reduce",
           "not_measured": "two gloo ranks stage through the host (a rehearsal path, no performance figure); RCCL at "
                           "world > 1 needs more than one GPU",
           "shapes": [measure(args.envs, args, dev)]}
    ref = os.path.join(ROOT, "profiles", "ppo_resident_ab.json")
    if os.path.exists(ref):               # the single-rank path against the figure recorded when it was built
        with open(ref) as f:
            for shape in json.load(f)["shapes"]:
                if (shape["envs"], shape["steps"]) == (args.envs, args.steps):
                    out["ppo_resident_ab_resident_wall"] = shape["sides"]["resident_wall"]
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
