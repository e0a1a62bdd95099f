"""cf2sim -- MI355X-native batched CrazyFlie hover environments (drop-in for the hover envs of
phoenix_drone_simulation, the package of Hu-Hanyang/disturbance-CrazyFile-simulation).

* ``BatchedCrazyflieEnv``: N envs per GPU, one fused HIP kernel per env-step (vec_env.py).
* ``make(id)``: single-env gym-style adapter with the reference's ids, spaces and 4-tuple API.
* ``cf2sim.physics``: the reference's physics plugin classes (``PybulletPhysicsWithAdversary``, ...,
  ``HipBatchedPhysics``) over the HIP physics kernel, for ``getattr(module, physics)`` lookups.
* ``solve_value_tables(cfg)``: the HJ-adversary envs' value tables, solved on the GPU (hj_solve.py).
* ``Population`` / ``collect_population`` / ``PopulationPPOUpdater`` / ``PopulationNaturalGradientUpdater``:
  P independent learners on one env batch, collected and updated (PPO, TRPO, NPG) with launch counts
  that do not depend on P (population.py).
"""
from .config import (ENV_SPECS, OUT_OF_SCOPE_IDS, REFERENCE_IDS, CF2Config, build_config,  # noqa: F401
                     spec_for_id)

__all__ = ["ENV_SPECS", "REFERENCE_IDS", "OUT_OF_SCOPE_IDS", "CF2Config", "build_config", "spec_for_id",
           "BatchedCrazyflieEnv", "make", "registry",
           "HJModel", "default_target", "time_step", "solve_value_table", "solve_value_tables", "save_value_tables",
           "Population", "PopulationRollout", "collect_population", "PopulationPPOUpdater",
           "PopulationNaturalGradientUpdater"]

_HJ_SOLVE = ("HJModel", "default_target", "time_step", "solve_value_table", "solve_value_tables", "save_value_tables")
_POPULATION = ("Population", "PopulationRollout", "collect_population", "PopulationPPOUpdater",
               "PopulationNaturalGradientUpdater")


def __getattr__(name):   # lazy: importing the package must not require torch / a GPU
    if name in _HJ_SOLVE:    # HJ value-table generation (hj_solve.py)
        from . import hj_solve
        return getattr(hj_solve, name)
    if name in _POPULATION:  # P independent learners on one env batch (population.py)
        from . import population
        return getattr(population, name)
    if name == "BatchedCrazyflieEnv":
        from .vec_env import BatchedCrazyflieEnv
        return BatchedCrazyflieEnv
    if name in ("make", "registry"):
        from . import registration
        return getattr(registration, name)
    raise AttributeError(name)
