"""The state snapshot round trip of the fp32 CPU restatement (oracle/: orc_get_state / orc_set_state),
on the protocol and the 24 cases of snapshot_util: the 16 compiled kernel instances and five
disturbance and level modes.  Every resynchronised GPU test loads the restatement through
orc_set_state; this file holds it to the property those tests assume, that an env loaded with a
snapshot continues exactly as the env that wrote it.

The snapshot goes through float32 on the way, as the public format does.  No tolerances: outputs,
the int rows and the kept float fields (parity_util.state_fields) of the final state are compared
with np.array_equal.  128 envs per case (132 in formations); the conditions of
snapshot_util.check_conditions hold at that count in every case.
"""
import numpy as np
import pytest

import oracle as O
from parity_util import copy_config, state_fields
from snapshot_util import CASES, actions, check_conditions, config, hj_tables, horizon, is_formation, reset_mask

N_CPU, N_CPU_FORMATION = 128, 132
OUTPUTS = ("obs", "rew", "done", "truncated", "cost", "level")


def _make(cfg):
    env = O.OracleEnv(copy_config(cfg), "f32")
    if cfg.disturbance == 5:            # HJ: tables are bound, not part of a snapshot
        V, tol = hj_tables()
        env.bind_tables(V, tol[:int(cfg.num_levels)])
    return env


def _export(env):
    """get_state() as the public format carries it: float32."""
    sf, si = env.get_state()
    return sf.astype(np.float32), si


def _step(env, a):
    obs, rew, done, info = env.step(a, want_final=True)
    return dict(obs=obs, rew=rew, done=done, truncated=info["truncated"], cost=info["cost"], level=info["level"],
                final_obs=info["final_obs"])


def _same_outputs(got, ref, what):
    for k in OUTPUTS:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k} differs"
    m = ref["done"]
    assert np.array_equal(got["final_obs"][m], ref["final_obs"][m]), f"{what}: final_obs differs"


def _same_state(env, ref, groups, what):
    (gf, gi), (rf, ri) = env.get_state(), ref.get_state()
    assert np.array_equal(gi, ri), f"{what}: int rows differ"
    for name, f in groups.items():
        assert np.array_equal(gf[f], rf[f]), f"{what}: float fields of {name} differ"


@pytest.mark.parametrize("label", list(CASES))
def test_restatement_snapshot_round_trip(label):
    n = N_CPU_FORMATION if is_formation(label) else N_CPU
    cfg = config(label, n)
    T, t0 = horizon(label)
    acts = actions(n, T)
    groups = state_fields(cfg)
    A, B, C = _make(cfg), _make(cfg), _make(cfg)
    assert np.array_equal(A.reset(), B.reset())
    done, trunc = np.zeros((T, n), bool), np.zeros((T, n), bool)
    for t in range(T):
        if t == t0:
            si_t0 = A.get_state()[1].copy()
            C.set_state(*_export(A))
            _same_state(C, A, groups, "fresh env, right after the import")
        B.set_state(*_export(B))
        ra = _step(A, acts[t])
        _same_outputs(_step(B, acts[t]), ra, f"re-imported env, env-step {t}")
        if t >= t0:
            _same_outputs(_step(C, acts[t]), ra, f"fresh env, env-step {t}")
        done[t], trunc[t] = ra["done"], ra["truncated"]
    for env, who in ((B, "re-imported env"), (C, "fresh env")):
        _same_state(env, A, groups, f"{who}, after env-step {T - 1}")
    mask = reset_mask(n)
    ro = A.reset(mask)
    for env, who in ((B, "re-imported env"), (C, "fresh env")):
        assert np.array_equal(env.reset(mask)[mask], ro[mask]), f"{who}: masked reset rows differ"
        _same_state(env, A, groups, f"{who}, after the masked reset")
    for env in (A, B, C):
        env.close()
    check_conditions(label, done, trunc, si_t0)
