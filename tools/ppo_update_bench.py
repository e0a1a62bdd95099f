"""Time the PPO gradient kernels at the headline update shape, in one process with the sides alternated
(device events; min / median / max over --repeats windows of --inner calls):
  policy_grad   cf2_ppo_policy_grad on all T N rows            vs torch fp32 autograd on policy_loss_torch
  value_grad    cf2_ppo_value_grad on all T N rows             vs torch fp32 autograd on value_loss_torch
  value_grad_mb one value mini-batch of 1/16 of the rows through idx_dev
                                                               vs torch on the gathered rows (gather included)
  policy_eval   the evaluate-only call of the KL check
The torch sides run loss + backward into .grad, as PPOUpdater(device=False) does; the kernel sides
write the flat gradient (scatter_flat_grad and the optimiser step are the same on both paths).
python tools/ppo_update_bench.py [--envs N] [--steps T] [--obs-dim D] [--out profiles/ppo_update_bench.json]"""
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
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--obs-dim", type=int, default=34)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from cf2sim import _native
    from cf2sim.ppo import policy_grad_device, policy_loss_torch, value_grad_device, value_loss_torch
    from cf2sim.rollout import MLPActorCritic, pack_policy_weights
    lib = _native.load()
    dev = torch.device("cuda", 0)
    n, d, clip = args.steps * args.envs, args.obs_dim, 0.2
    g = torch.Generator(device=dev).manual_seed(0)
    torch.manual_seed(0)
    ac = MLPActorCritic(obs_dim=d).to(dev)
    obs = torch.randn(n, d, device=dev, generator=g)
    with torch.no_grad():
        act, _, logp_old = ac.step(obs, generator=g)
        logp_old = logp_old + 0.2 * torch.randn(n, device=dev, generator=g)      # ratios on both sides of the clip range
    adv = torch.randn(n, device=dev, generator=g)
    target = torch.randn(n, device=dev, generator=g)
    flat = pack_policy_weights(ac)
    grad = torch.zeros_like(flat)
    summary = torch.zeros(8, dtype=torch.float64, device=dev)
    scratch = torch.empty((lib.cf2_ppo_scratch_bytes(n, d) + 7) // 8, dtype=torch.float64, device=dev)
    mb = n // 16
    idx64 = torch.randperm(n, device=dev, generator=g)[:mb]
    idx = idx64.to(torch.int32)

    def torch_side(loss):
        def run():
            for p in ac.parameters():
                p.grad = None
            loss().backward()
        return run

    sides = {
        "policy_grad": lambda: policy_grad_device(flat, obs, act, logp_old, adv, clip, summary, scratch, grad=grad),
        "policy_grad_torch": torch_side(lambda: policy_loss_torch(ac, obs, act, logp_old, adv, clip)),
        "value_grad": lambda: value_grad_device(flat, obs, target, summary, scratch, grad=grad),
        "value_grad_torch": torch_side(lambda: value_loss_torch(ac, obs, target)),
        "value_grad_mb": lambda: value_grad_device(flat, obs, target, summary, scratch, grad=grad, idx=idx),
        "value_grad_mb_torch": torch_side(lambda: value_loss_torch(ac, obs[idx64], target[idx64])),
        "policy_eval": lambda: policy_grad_device(flat, obs, act, logp_old, adv, clip, summary, scratch),
    }
    for fn in sides.values():             # warm up every shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):         # the sides alternate inside every repeat
        for k, fn in sides.items():
            times[k].append(window_us(fn, args.inner))
    res = {k: {"min_us": min(v), "median_us": statistics.median(v), "max_us": max(v)} for k, v in times.items()}
    med = {k: r["median_us"] for k, r in res.items()}
    # multiply-adds of forward, backward into the activations (not into the observation) and weight
    # gradient, 2 FLOP each, from the shapes
    mac = lambda h, no: d * h + h * h + h * no
    flop = {"policy_grad": 2 * n * (3 * mac(50, 4) - d * 50), "value_grad": 2 * n * (3 * mac(64, 1) - d * 64)}
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "obs_dim": d, "mini_batch_rows": mb,
           "repeats": args.repeats, "calls_per_window": args.inner, "timing": "device events, sides alternated",
           "sides": res,
           "torch_over_kernel": {k: med[k + "_torch"] / med[k] for k in ("policy_grad", "value_grad", "value_grad_mb")},
           "kernel_tflops_useful": {k: flop[k] / med[k] * 1e-6 for k in flop}}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
