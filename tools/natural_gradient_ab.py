"""A/B of the natural-gradient update (TRPO; cg_iters = 10, every fourth row in the Fisher-vector
product), in one process with the sides alternated (min / median / max over --repeats windows):

per update   NaturalGradientUpdater(device=True)  -- the resident launch sequence, one host read at the end
             NaturalGradientUpdater(device=False) -- the same loop through torch autograd (double backward
             for the Fisher-vector product) and torch.optim.Adam, on the GPU in fp32
             on the same synthetic rollout from the same starting weights (reloaded before every window,
             outside the timed span).  The torch side reads the host at every line-search trial, so the
             common clock is the host's around updates that end in a device read; the device side is also
             timed with device events around ``update(read=False)``.
per launch   cf2_ppo_fisher_vec against cf2_ppo_policy_grad with a gradient on the same m rows through the
             same index, and against fisher_vec_torch in fp32 on the GPU on the gathered rows; device
             events around --launches launches each, the three alternated.

python tools/natural_gradient_ab.py [--shapes 32768,262144] [--steps 32] [--out profiles/natural_gradient_ab.json]"""
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


def synthetic(envs, T, d, dev):
    from cf2sim.rollout import MLPActorCritic, Rollout
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
    return ac, ro


def measure_update(envs, args, dev):
    from cf2sim.ppo import NaturalGradientUpdater
    ac, ro = synthetic(envs, args.steps, args.obs_dim, dev)
    start = copy.deepcopy(ac.state_dict())
    kw = dict(algorithm="trpo", cg_iters=args.cg_iters, fvp_stride=args.stride, train_v_iterations=args.v_iters)
    mk = lambda device: NaturalGradientUpdater(ac, 1e-3, args.target_kl, device=device,
                                               generator=torch.Generator(device=dev).manual_seed(1), **kw)
    device, torch_side = mk(True), mk(False)

    def window(side):
        ac.load_state_dict(start)
        torch.cuda.synchronize()
        if side == "events":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            device.update(ro, read=False)
            e1.record()
            enq = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            return {"device_events": e0.elapsed_time(e1), "device_enqueue": enq}, device.result()
        up = device if side == "device" else torch_side
        t0 = time.perf_counter()
        out = up.update(ro)
        return {side + "_wall": (time.perf_counter() - t0) * 1e3}, out

    sides = ("device", "torch", "events")
    last, times = {}, {}
    for s in sides:                       # warm up every shape and path
        _, last[s] = window(s)
    for _ in range(args.repeats):         # the sides alternate inside every repeat
        for s in sides:
            t, last[s] = window(s)
            for k, v in t.items():
                times.setdefault(k, []).append(v)
    res = {k: stats(v) for k, v in times.items()}
    return {"envs": envs, "steps": args.steps, "rows": args.steps * envs, "fvp_rows": -(-args.steps * envs // args.stride),
            "sides": res, "torch_over_device_wall": res["torch_wall"]["median_ms"] / res["device_wall"]["median_ms"],
            "last_update": {"device": last["device"], "torch": last["torch"]}}


def measure_launch(envs, args, dev):
    from cf2sim import _native
    from cf2sim.ppo import fisher_vec_device, fisher_vec_torch, flat_slice, policy_grad_device
    from cf2sim.rollout import pack_policy_weights
    lib = _native.load()
    ac, ro = synthetic(envs, args.steps, args.obs_dim, dev)
    d = args.obs_dim
    obs, act = ro.obs.reshape(-1, d).contiguous(), ro.act.reshape(-1, 4).contiguous()
    lpo, adv = ro.logp.reshape(-1).contiguous(), ro.adv.reshape(-1).contiguous()
    n = obs.shape[0]
    idx = torch.arange(0, n, args.stride, dtype=torch.int32, device=dev)
    m = idx.shape[0]
    sub = obs[::args.stride].contiguous()
    flat = pack_policy_weights(ac)
    vec = torch.randn_like(flat) * 0.05
    out, grad = torch.zeros_like(flat), torch.zeros_like(flat)
    summary = torch.zeros(8, dtype=torch.float64, device=dev)
    scratch = torch.empty((lib.cf2_ppo_scratch_bytes(n, d) + 7) // 8, dtype=torch.float64, device=dev)
    v_pi = vec[:flat_slice(ac, "pi")[1]]
    sides = {
        "fisher_vec": lambda: fisher_vec_device(flat, obs, vec, out, summary, scratch, idx=idx),
        "policy_grad": lambda: policy_grad_device(flat, obs, act, lpo, adv, float("inf"), summary, scratch, grad=grad,
                                                  idx=idx),
        "fisher_vec_torch": lambda: fisher_vec_torch(ac, sub, v_pi),
    }
    times = {}
    for k, fn in sides.items():           # warm up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.setdefault(k, []).append(e0.elapsed_time(e1) / args.launches)
    res = {k: stats(v) for k, v in times.items()}
    med = lambda k: res[k]["median_ms"]
    return {"rows": n, "m": m, "per_launch": res, "fisher_over_policy_grad": med("fisher_vec") / med("policy_grad"),
            "torch_over_fisher": med("fisher_vec_torch") / med("fisher_vec")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32768,262144", help="envs per rollout, comma separated")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--obs-dim", type=int, default=34)
    ap.add_argument("--cg-iters", type=int, default=10)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--v-iters", type=int, default=5)
    ap.add_argument("--target-kl", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "natural_gradient_ab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    shapes = [int(e) for e in args.shapes.split(",")]
    out = {"device": torch.cuda.get_device_name(0), "obs_dim": args.obs_dim, "algorithm": "trpo", "cg_iters": args.cg_iters,
           "fvp_stride": args.stride, "v_iterations": args.v_iters, "mini_batches": 16, "target_kl": args.target_kl,
           "line_search_steps": 25, "repeats": args.repeats, "launches_per_window": args.launches,
           "timing": "per update: host clock around one update that ends in a device read (wall), device events around "
                     "update(read=False) (events), host time of that call (enqueue); per launch: device events around "
                     "launches_per_window launches; one warm-up window per side, sides alternated",
           "updates": [measure_update(e, args, dev) for e in shapes],
           "launches": [measure_launch(e, args, dev) for e in shapes]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
