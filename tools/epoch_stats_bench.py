"""Time the per-epoch statistics kernels at the headline collect shape, in one process with the sides
alternated (device events; min / median / max over --repeats windows of --inner calls):
  (i)  cf2_column_moments on [T N, D] f32 vs cf2_hbm_probe(mode=1) over the same bytes (the read
       stream the kernel should approach) and vs OnlineMeanStd.update on the same tensor (torch);
       also the [T N] discounted returns (D = 1);
  (ii) cf2_episode_stats on [T, N] rew / done, with and without cost, its bytes over the probe rate.
The small inputs of (ii) and of D = 1 rotate over enough buffer sets to exceed the 256 MiB cache.
python tools/epoch_stats_bench.py [--envs N] [--steps T] [--obs-dim D] [--out FILE]"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--obs-dim", type=int, default=34)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from cf2sim import _native
    from cf2sim.rollout import OnlineMeanStd
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    T, n, d = args.steps, args.envs, args.obs_dim
    rows = T * n
    g = torch.Generator(device=dev).manual_seed(0)

    # (i) column moments
    x = torch.randn(rows, d, device=dev, generator=g)
    xbytes = x.numel() * 4
    assert xbytes % 16 == 0
    sink = torch.empty(4096, dtype=torch.uint8, device=dev)
    out = torch.empty(2 * d, dtype=torch.float64, device=dev)
    scratch = torch.empty(lib.cf2_column_moments_scratch_bytes(rows, d) // 8, dtype=torch.float64, device=dev)
    nsets = max(2, -(-(320 << 20) // (rows * 4)))
    rets = [torch.randn(rows, device=dev, generator=g) for _ in range(nsets)]
    out1 = torch.empty(2, dtype=torch.float64, device=dev)
    scratch1 = torch.empty(lib.cf2_column_moments_scratch_bytes(rows, 1) // 8, dtype=torch.float64, device=dev)
    oms = OnlineMeanStd(shape=(d,)).to(dev)

    def probe(_):
        _native.check(lib.cf2_hbm_probe(sink.data_ptr(), x.data_ptr(), xbytes, 1, stream), "cf2_hbm_probe")

    def moments(_):
        _native.check(lib.cf2_column_moments(x.data_ptr(), rows, d, out.data_ptr(), scratch.data_ptr(), stream),
                      "cf2_column_moments")

    def moments1(i):
        _native.check(lib.cf2_column_moments(rets[i % nsets].data_ptr(), rows, 1, out1.data_ptr(), scratch1.data_ptr(),
                                             stream), "cf2_column_moments")

    def torch_update(_):
        oms.update(x)

    def device_update(_):
        oms.update_device(x)

    # (ii) episode statistics
    esets = max(2, -(-(320 << 20) // (rows * 5)))
    rews = [torch.randn(T, n, device=dev, generator=g) for _ in range(esets)]
    costs = [torch.randn(T, n, device=dev, generator=g) for _ in range(esets)]
    dones = [(torch.rand(T, n, device=dev, generator=g) < 0.002).to(torch.uint8) for _ in range(esets)]   # 1 / 500 steps
    cr, cc = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    cl = torch.zeros(n, dtype=torch.int32, device=dev)
    summary = torch.zeros(16, dtype=torch.float64, device=dev)
    escratch = torch.empty(lib.cf2_episode_stats_scratch_bytes(n) // 8, dtype=torch.float64, device=dev)

    def episode(with_cost):
        def run(i):
            k = i % esets
            _native.check(lib.cf2_episode_stats(T, n, rews[k].data_ptr(), costs[k].data_ptr() if with_cost else None,
                                                dones[k].data_ptr(), cr.data_ptr(), cc.data_ptr(), cl.data_ptr(), None,
                                                None, None, summary.data_ptr(), 1, escratch.data_ptr(), stream),
                          "cf2_episode_stats")
        return run

    sides = {"hbm_probe_read": (probe, args.inner), "column_moments": (moments, args.inner),
             "torch_update": (torch_update, max(2, args.inner // 20)),
             "update_device": (device_update, args.inner),
             "column_moments_d1": (moments1, args.inner),
             "episode_stats": (episode(False), args.inner), "episode_stats_cost": (episode(True), args.inner)}
    for fn, _ in sides.values():          # warm up every shape
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):         # the sides alternate inside every repeat
        for k, (fn, inner) in sides.items():
            times[k].append(window_us(fn, inner))

    med = {k: statistics.median(v) for k, v in times.items()}
    probe_rate = xbytes / med["hbm_probe_read"]          # bytes per us
    ep_bytes = rows * 5 + n * 24                         # rew + done, carries read and written
    ep_bytes_cost = ep_bytes + rows * 4
    lines = [f"epoch statistics kernels, {torch.cuda.get_device_name(0)}; T = {T}, N = {n}, D = {d}; "
             f"{args.repeats} repeats, sides alternated, device events",
             f"{'side':<22}{'calls/window':>13}{'min us':>12}{'median us':>12}{'max us':>12}"]
    for k, v in times.items():
        lines.append(f"{k:<22}{sides[k][1]:>13}{min(v):>12.1f}{med[k]:>12.1f}{max(v):>12.1f}")
    lines += [
        f"matrix bytes {xbytes} ({xbytes / 1e9:.3f} GB); read-probe rate {probe_rate * 1e-6:.3f} TB/s (median)",
        f"column_moments [{rows}, {d}]: {xbytes / med['column_moments'] * 1e-6:.3f} TB/s = "
        f"{xbytes / med['column_moments'] / probe_rate * 100:.1f} % of the measured read-probe rate",
        f"column_moments vs torch OnlineMeanStd.update: {med['torch_update'] / med['column_moments']:.2f}x faster "
        f"(update_device, moments + the fp64 update ops: {med['torch_update'] / med['update_device']:.2f}x)",
        f"column_moments [{rows}] (D = 1, {nsets} buffers in rotation): {rows * 4 / med['column_moments_d1'] * 1e-6:.3f} "
        f"TB/s = {rows * 4 / med['column_moments_d1'] / probe_rate * 100:.1f} % of the read-probe rate",
        f"episode_stats [{T}, {n}] without cost ({esets} buffer sets in rotation): {ep_bytes} B, "
        f"{ep_bytes / med['episode_stats'] * 1e-6:.3f} TB/s = {ep_bytes / med['episode_stats'] / probe_rate * 100:.1f} % "
        f"of the read-probe rate",
        f"episode_stats [{T}, {n}] with cost: {ep_bytes_cost} B, {ep_bytes_cost / med['episode_stats_cost'] * 1e-6:.3f} "
        f"TB/s = {ep_bytes_cost / med['episode_stats_cost'] / probe_rate * 100:.1f} % of the read-probe rate",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
