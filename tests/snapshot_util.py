"""Shared by test_snapshot_roundtrip_cpu.py and test_snapshot_roundtrip_gpu.py: the cases of the
state snapshot round trip (cf2_get_state -> cf2_set_state -> env-steps), their horizons and the
conditions that keep a run from passing vacuously.

Protocol (three envs of one configuration, the same actions):
  A  reset once, never imported: the reference;
  B  reset once; before every env-step it exports its state and imports it again;
  C  constructed and never reset (what from_checkpoint does); before env-step t0 it imports A's
     export and steps from there.
Every output of B at every env-step, and of C from env-step t0 on, equals A's bit for bit, and so
do the exported states after the last env-step and after a masked reset of every third env.
"""
import functools

import numpy as np

from cf2sim.config import build_config
from parity_util import wide_actions
from test_gpu_large_kernels import CASES as LARGE_CASES

SEED = 3
ACTION_SEED = 17
I_EP_STEP, I_RNG, I_FLAGS, I_LEVEL, I_GUST = range(5)

# disturbance and level modes on the default shape, next to the 16 compiled instances of LARGE_CASES
MODES = {
    "hj-fixed": "DroneHoverBulletFreeEnvWithAdversary-v0",
    "hj-boltzmann": "DroneHoverBulletFreeEnvWithRandomHJAdversary-v0",
    "hj-initial": "DroneHoverBulletFreeEnvWithAdversaryInitial-v0",
    "uniform": "DroneHoverBulletFreeEnvWithRandomAdversary-v0",
    "const-wind": "DroneHoverBulletFreeEnvWithConstWind-v0",
}
# label -> (env id, kwargs); the env counts and horizons of LARGE_CASES are not used
CASES = {label: (env_id, kw) for label, (env_id, _, _, kw) in LARGE_CASES.items()}
CASES.update({label: (env_id, {}) for label, env_id in MODES.items()})
assert len(CASES) == len(LARGE_CASES) + len(MODES)
FUSED_CASES = ("s1-n1d1-gust", "hj-boltzmann", "const-wind")


def horizon(label):
    """(T, t0): env-steps of the run and the env-step before which C imports A's state."""
    return (60, 20) if CASES[label][1].get("aggregate_phy_steps") == 1 else (24, 9)


def is_formation(label):
    return "Downwash" in CASES[label][0]


def config(label, n):
    env_id, kw = CASES[label]
    return build_config(env_id, n, seed=SEED, **kw)


def actions(n, T):
    """[T, n, 4] float32, drawn step by step from one generator."""
    rng = np.random.default_rng(ACTION_SEED)
    return np.stack([wide_actions(rng, n) for _ in range(T)])


@functools.lru_cache(maxsize=1)
def hj_tables():
    """The value tables every HJ env of a trio binds (tables are not part of a snapshot):
    (V [3, 15^6] float32, table_of_level for 32 levels, cut to cfg.num_levels by the caller)."""
    from test_gpu_parity import _synthetic_tables
    return _synthetic_tables(range(3), seed=1).reshape(3, -1), [lv % 3 for lv in range(32)]


def reset_mask(n):
    return np.arange(n) % 3 == 0


def check_conditions(label, done, trunc, si_t0):
    """The conditions on A's own outputs: done / trunc [T, n] bool of every env-step, si_t0 [5, n]
    the int rows of A's state before env-step t0.  Returns the printed report line."""
    T, t0 = horizon(label)
    env_id, kw = CASES[label]
    n = done.shape[1]
    assert done.shape[0] == T
    per_step = done[t0 + 1:].sum(1)
    line = (f"{label} ({n} envs): auto-resets after env-step {t0}: {int(per_step.sum())} over {T - t0 - 1} env-steps, "
            f"largest in one step {int(per_step.max())}")
    print(line)
    assert per_step.sum() > 0, "no auto-reset after the import"
    if kw.get("max_episode_steps") == 7:
        full = [t for t in range(t0 + 1, T) if done[t].all()]
        assert full and all(trunc[t].all() for t in full), "no env-step after the import times every env out"
    else:
        assert ((per_step > 0) & (per_step < n)).any(), "no env-step after the import resets some but not all envs"
    if "Gust" in env_id:
        in_gust = int((si_t0[I_GUST] > 0).sum())
        print(f"{label}: {in_gust} of {n} envs in a gust at the import")
        assert 0 < in_gust < n
    if label == "hj-boltzmann":
        levels = len(np.unique(si_t0[I_LEVEL]))
        print(f"{label}: {levels} distinct level indices at the import")
        assert levels >= 3
    if label == "const-wind" or label.startswith("hj-"):
        ep = si_t0[I_EP_STEP]
        print(f"{label}: ep_step at the import spans {int(ep.min())} to {int(ep.max())}")
        assert (ep == 0).any() and (ep > 0).any(), "no env at ep_step 0 next to envs mid-episode at the import"
    return line
