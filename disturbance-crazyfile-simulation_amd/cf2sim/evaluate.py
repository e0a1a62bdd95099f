"""Policy evaluation per disturbance level: the reference's ``utils/evaluation.py`` / ``play.py``
(run a trained ActorCritic for a number of episodes and report returns, lengths and costs) for a
batch of envs that auto-reset on the device.

A loop that simply counts every finished episode of auto-resetting envs is biased towards short
episodes: an env that crashes after 20 steps contributes 25 episodes in the time a surviving one
contributes one.  ``evaluate`` therefore gives every env a quota (``LevelOutcomes.set_quota``):
exactly ``episodes_per_env`` episodes of each env are recorded, the first ones it finishes, and
the loop runs until every quota is used up.  The TimeLimit bounds that: an episode lasts at most
``max_episode_steps`` env-steps, so E episodes per env are over after E * max_episode_steps steps.

The loop makes two launches per env-step (``envs.step_into`` and ``ac.step``); the fused collect
kernels always sample, and an evaluation's time does not matter.

Command line::

    python -m cf2sim.evaluate --env ID --num-envs N --weights FILE.pt [--tables DIR] [--episodes E]
                              [--stochastic] [--uniform-levels] [--seed S] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import math

import torch


def chunk_bound(episodes_per_env: int, max_episode_steps: int, chunk: int) -> int:
    """Chunks of ``chunk`` env-steps after which every env has finished ``episodes_per_env`` episodes:
    ceil(E * max_episode_steps / chunk) (an episode ends at the TimeLimit at the latest)."""
    e, m, c = int(episodes_per_env), int(max_episode_steps), int(chunk)
    if e < 1 or c < 1:
        raise ValueError(f"episodes_per_env and chunk must be positive, got {episodes_per_env}, {chunk}")
    if m < 1:
        raise ValueError("evaluate() needs a TimeLimit (max_episode_steps > 0): without one an episode may never end")
    return -(-e * m // c)


@torch.no_grad()
def evaluate(envs, ac, episodes_per_env: int = 1, deterministic: bool = True, chunk: int = 32) -> dict:
    """Run ``ac`` (a FusedActorCritic or an MLPActorCritic) in ``envs`` from a reset until every env
    has finished ``episodes_per_env`` episodes, and return ``LevelOutcomes.table_of`` of exactly those
    episodes (per level: episodes, crashes, time-outs, crash rate, EpRet / EpLen / EpCosts) plus
    ``"env_steps"`` and ``"chunks"``, the steps and chunks the loop ran, and ``"raw"``, the [L + 1][16]
    table itself as lists (``LevelOutcomes.merge_raw`` combines the ranks').  deterministic: the policy's
    mean action (the reference's evaluation) instead of a sample.  The envs are left wherever the
    last chunk ended; reset them before training on."""
    from .rollout import FusedActorCritic, LevelOutcomes
    n, d, dev = envs.num_envs, envs.obs_dim, envs.device
    bound = chunk_bound(episodes_per_env, int(envs.cfg.max_episode_steps), chunk)
    if not bool(envs.cfg.auto_reset):
        raise ValueError("evaluate() needs auto-resetting envs")
    outcomes = LevelOutcomes.for_env(envs)
    outcomes.set_quota(episodes_per_env)
    obs = envs.reset()
    nxt = [torch.empty(n, d, device=dev), torch.empty(n, d, device=dev)]      # step_into's obs, alternating
    rew, cost, level = (torch.empty(chunk, n, device=dev) for _ in range(3))
    done, trunc = (torch.empty(chunk, n, dtype=torch.uint8, device=dev) for _ in range(2))
    kw = {"row_offset": int(envs.cfg.env_id_offset)} if isinstance(ac, FusedActorCritic) else {}
    chunks = 0
    while chunks < bound:
        for t in range(chunk):
            act = ac.step(obs, deterministic=deterministic, **kw)[0].contiguous()
            o = nxt[t & 1]
            envs.step_into(act, o, rew[t], done[t], trunc[t], cost[t], level_out=level[t])
            obs = o
        outcomes.update(rew, done, trunc, cost, level)
        chunks += 1
        if outcomes.remaining() == 0:
            break
    left = outcomes.remaining()
    if left:
        raise RuntimeError(f"{left} episodes still running after {chunks} chunks of {chunk} steps: the TimeLimit "
                           f"({int(envs.cfg.max_episode_steps)} steps) should have ended them")
    raw = outcomes.raw().cpu()
    out = outcomes.summary()
    out["env_steps"], out["chunks"], out["raw"] = chunks * chunk, chunks, raw.tolist()
    return out


def load_policy(path: str, obs_dim: int, device):
    """An MLPActorCritic from a ``state_dict`` file: this package's, or the reference's ActorCritic
    (keys pi.net.*, v.net.*, pi.log_std: ``MLPActorCritic.load_reference_state_dict``).  The file is
    read with ``weights_only=True``: tensors only, nothing in it is executed."""
    from .rollout import MLPActorCritic
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path} does not hold a state_dict")
    ac = MLPActorCritic(obs_dim=obs_dim)
    if "pi.net.0.weight" in sd:
        ac.load_reference_state_dict(sd)
    else:
        ac.load_state_dict(sd)
    return ac.to(device)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m cf2sim.evaluate", description="Evaluate a policy per disturbance level.")
    p.add_argument("--env", required=True, help="registered env id")
    p.add_argument("--num-envs", type=int, required=True)
    p.add_argument("--weights", required=True, help="state_dict of MLPActorCritic or of the reference's ActorCritic")
    p.add_argument("--tables", default=None, help="directory of the HJ value tables (fastrack_{level}_15x15.npy)")
    p.add_argument("--episodes", type=int, default=1, help="episodes per env")
    p.add_argument("--stochastic", action="store_true", help="sample actions instead of taking the mean")
    p.add_argument("--uniform-levels", action="store_true",
                   help="draw every disturbance level with the same probability (Boltzmann-level envs)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--chunk", type=int, default=32, help="env-steps between two checks of the quota")
    p.add_argument("--out", default=None, help="write the result as JSON to this file instead of stdout")
    return p


def _jsonable(x):
    """NaN and infinities (statistics of an empty level) as null: strict JSON has no such numbers"""
    if isinstance(x, dict):
        return {k: _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, float) and not math.isfinite(x):
        return None
    return x


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if args.num_envs < 1 or args.episodes < 1 or args.chunk < 1:
        raise SystemExit("--num-envs, --episodes and --chunk must be positive")
    from .rollout import FusedActorCritic
    from .vec_env import BatchedCrazyflieEnv
    envs = BatchedCrazyflieEnv(args.env, args.num_envs, seed=args.seed, value_tables=args.tables)
    if args.uniform_levels:
        envs.set_level_distribution([1.0] * int(envs.cfg.num_levels))
    ac = FusedActorCritic(load_policy(args.weights, envs.obs_dim, envs.device), seed=args.seed)
    res = evaluate(envs, ac, episodes_per_env=args.episodes, deterministic=not args.stochastic, chunk=args.chunk)
    res.update({"env": args.env, "num_envs": args.num_envs, "episodes_per_env": args.episodes,
                "deterministic": not args.stochastic, "uniform_levels": bool(args.uniform_levels)})
    text = json.dumps(_jsonable(res), indent=1, allow_nan=False)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    envs.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
