"""A/B of the whole PPO update, in one process with the sides alternated (windows of --inner whole
``update`` calls; min / median / max over --repeats windows):
  parent     PPOUpdater(device=True) with torch.optim.Adam: per policy iteration a gradient pass, the
             scatter into .grad, the optimiser step, the re-pack, an evaluate-only pass and a host read
  resident   ResidentPPOUpdater: one pass per iteration, cf2_adam_step on the flat block, the KL stop
             on the device, one host read at the end
target_kl = 1e9, so both run all --pi-iters policy iterations and --v-iters x 16 value mini-batches on
the same synthetic rollout from the same starting weights (reloaded before every window, outside the
timed span).  The parent synchronises every iteration, so the common clock is the host's around
updates that end in a device read; the resident side is also timed with device events around
``update(read=False)`` calls, and its enqueue time (the host's share, nothing waited for) is reported.
python tools/ppo_resident_ab.py [--shapes 32768,262144] [--steps 32] [--out profiles/ppo_resident_ab.json]"""
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
    from cf2sim.ppo import PPOUpdater, ResidentPPOUpdater
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
    parent = PPOUpdater(ac, torch.optim.Adam(ac.pi_net.parameters(), lr=3e-4),
                        torch.optim.Adam(ac.v_net.parameters(), lr=1e-3), 0.2, 1e9, device=True,
                        generator=torch.Generator(device=dev).manual_seed(1), **kw)
    resident = ResidentPPOUpdater(ac, 3e-4, 1e-3, 0.2, 1e9, generator=torch.Generator(device=dev).manual_seed(1), **kw)

    def window(side):
        ac.load_state_dict(start)
        torch.cuda.synchronize()
        if side == "parent":
            t0 = time.perf_counter()
            for _ in range(args.inner):
                out = parent.update(ro)
            return {"parent_wall": (time.perf_counter() - t0) / args.inner * 1e3}, out
        if side == "resident":
            t0 = time.perf_counter()
            for _ in range(args.inner):
                out = resident.update(ro)
            return {"resident_wall": (time.perf_counter() - t0) / args.inner * 1e3}, out
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.inner):
            resident.update(ro, read=False)
        e1.record()
        enq = (time.perf_counter() - t0) / args.inner * 1e3
        torch.cuda.synchronize()
        return {"resident_device": e0.elapsed_time(e1) / args.inner, "resident_enqueue": enq}, resident.result()

    sides = ("parent", "resident", "resident_events")
    last = {}
    for s in sides:                       # warm up every shape and path
        _, last[s] = window(s)
    times = {}
    for _ in range(args.repeats):         # the sides alternate inside every repeat
        for s in sides:
            t, last[s] = window(s)
            for k, v in t.items():
                times.setdefault(k, []).append(v)
    res = {k: stats(v) for k, v in times.items()}
    assert last["parent"]["StopIter"] == last["resident"]["StopIter"] == args.pi_iters
    return {"envs": envs, "steps": T, "rows": T * envs, "sides": res,
            "parent_over_resident_wall": res["parent_wall"]["median_ms"] / res["resident_wall"]["median_ms"],
            "last_update": {"parent": last["parent"], "resident": last["resident"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32768,262144", help="envs per rollout, comma separated")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--obs-dim", type=int, default=34)
    ap.add_argument("--pi-iters", type=int, default=80)
    ap.add_argument("--v-iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_resident_ab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "obs_dim": args.obs_dim, "pi_iterations": args.pi_iters,
           "v_iterations": args.v_iters, "mini_batches": 16, "target_kl": 1e9, "repeats": args.repeats,
           "updates_per_window": args.inner,
           "timing": "host clock around updates that end in a device read (wall), device events around "
                     "update(read=False) (device), host time of those calls (enqueue); sides alternated",
           "shapes": [measure(int(e), args, dev) for e in args.shapes.split(",")]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
