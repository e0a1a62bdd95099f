"""The store cache policy of the large-N env kernels (CF2SIM_STORE_POLICY, cf2_store_policy;
DESIGN.md section 3): the parser and the automatic choice without a GPU, and on the GPU that every
policy the library compiles gives bit-identical results to the plain one: every output of every
env-step and the state snapshot after the last, in runs whose resets make two waves store the same
state groups in one launch.  (step_kernel alone takes the policy: the small-N kernels, collect_kernel
and rollout_kernel have one form, profiles/store_policy_ab.txt.)"""
import os

import numpy as np
import pytest
import torch

from cf2sim.config import build_config
from parity_util import N1, SMALL_N_MAX, wide_actions

GUST = "DroneHoverBulletFreeEnvWithGust-v0"     # the bench workload (C4): reference-default shape, SPEC 1
SIMPLE = "DroneHoverSimpleEnv-v0"               # SimplePhysics: a generic (SPEC 0) instance
PLAIN, NT, WT, NT_WT = 0, 2, 16, 18             # include/cf2sim.h CF2_STORE_*
NAMES = {"plain": PLAIN, "nt": NT, "wt": WT, "nt_wt": NT_WT}
# (state, obs, out) policies the library has large-N kernel instances for, by their override text
COMPILED = {
    "plain": (PLAIN, NT, PLAIN),
    "nt": (NT, NT, PLAIN),
    "wt": (WT, NT_WT, PLAIN),
}
NT_STATE_BYTES = 240 << 20                      # csrc/cf2sim_api.cpp
BENCH_STEP_BYTES = 762                          # step_bytes_per_env of the bench workload (bench.py counts the same)


def auto_policy(n, step_bytes=BENCH_STEP_BYTES):
    """Python mirror of choose_store_policy (csrc/cf2sim_api.cpp); checked against the library below."""
    if n <= SMALL_N_MAX:
        return (PLAIN, NT, PLAIN)           # the small-N kernels' one policy
    if n * step_bytes <= NT_STATE_BYTES:
        return (WT, NT_WT, PLAIN)           # cache-resident: write-through
    return (NT, NT, PLAIN)                  # beyond the Infinity Cache


def step_bytes(c):
    """Python mirror of step_bytes_per_env (csrc/cf2sim_api.cpp): bytes one env-step moves per env."""
    noise, dr = bool(c.observation_noise_on), bool(c.domain_randomization_on)
    ol, B = (13 if noise else 17), int(c.buf_size)
    held = c.aggregate_phy_steps % c.obs_rate != 0
    gust, const, hj = c.disturbance == 4, c.disturbance == 3, c.disturbance == 5
    level = const or hj or c.level_mode == 1
    persist = 13 + 8 + 4 * B + (6 if noise else 0) + (10 if noise and held else 0) + ol + 8
    persist += (3 if c.physics == 1 else 0) + (4 if c.use_motor_dynamics else 0)
    rd_f = persist + (15 if dr else 0) + (3 if gust or const else 0) + (1 if level else 0)
    wr_f = persist + (3 if gust else 0)
    rd_i, wr_i = 3 + (1 if level else 0) + (1 if gust else 0), 3 + (1 if gust else 0)
    b = 4 * (rd_f + wr_f + rd_i + wr_i) + 16 + (12 if c.disturbance == 1 else 0)
    return b + 4 * 2 * (ol + 4) + 4 + 1 + 1 + 4 + 4


@pytest.fixture(scope="module")
def native():
    from cf2sim.build import build_native
    build_native()
    from cf2sim import _native
    _native.load()
    return _native


def test_parser_accepts_every_documented_form(native):
    cfg = build_config(GUST, N1)
    assert native.store_policy_for(cfg, "plain") == (PLAIN, NT, PLAIN)
    assert native.store_policy_for(cfg, "nt") == (NT, NT, PLAIN)
    assert native.store_policy_for(cfg, "wt") == (WT, NT_WT, PLAIN)
    assert native.store_policy_for(cfg, "auto") == native.store_policy_for(cfg, "") == auto_policy(N1)
    # the three-part form: any subset, any order; parts left out keep the plain policy's value
    assert native.store_policy_for(cfg, "state=wt,obs=nt_wt,out=plain") == (WT, NT_WT, PLAIN)
    assert native.store_policy_for(cfg, "out=plain,obs=nt_wt,state=wt") == (WT, NT_WT, PLAIN)
    assert native.store_policy_for(cfg, "state=nt") == (NT, NT, PLAIN)
    assert native.store_policy_for(cfg, "obs=nt") == (PLAIN, NT, PLAIN)
    # well-formed, but no kernel instance: refused, never replaced by another policy
    for text in ("state=wt", "obs=nt_wt", "out=wt", "state=nt_wt,obs=nt_wt"):
        with pytest.raises(native.CF2Error, match="unsupported"):
            native.store_policy_for(cfg, text)


@pytest.mark.parametrize("junk", ["fast", "WT", "plain ", " wt", "wt,nt", "state", "state=", "state=sc1", "state=wt,",
                                  ",state=wt", "state=wt,state=nt", "rows=wt", "state=wt;obs=nt", "obs=nt_wt_", "=wt",
                                  "16"])
def test_parser_rejects_junk(native, junk):
    with pytest.raises(native.CF2Error, match="invalid argument"):
        native.store_policy_for(build_config(GUST, N1), junk)


def test_compiled_policies_are_the_documented_ones(native):
    """Exactly the policies of COMPILED have kernel instances: any other well-formed one is refused as
    unsupported (a missing kernel is an error, never another policy run quietly)."""
    cfg = build_config(GUST, N1)
    got = set()
    for s, sv in NAMES.items():
        for o, ov in NAMES.items():
            for u, uv in NAMES.items():
                text = f"state={s},obs={o},out={u}"
                try:
                    assert native.store_policy_for(cfg, text) == (sv, ov, uv)
                    got.add((sv, ov, uv))
                except native.CF2Error as e:
                    assert "unsupported" in str(e), text
    assert got == set(COMPILED.values())
    for text, pol in COMPILED.items():
        assert native.store_policy_for(cfg, text) == pol, text


def test_automatic_choice_by_regime(native):
    """Both sides of SMALL_N_MAX and of the NT_STATE_BYTES boundary of the bench configuration; the
    small-N kernels have one compiled policy, whatever the override asks for."""
    edge = NT_STATE_BYTES // BENCH_STEP_BYTES           # the last env count whose working set still fits
    assert SMALL_N_MAX < edge < (1 << 20)
    for n in (300, SMALL_N_MAX, SMALL_N_MAX + 1, N1, 262144, edge, edge + 1, 1 << 20):
        assert native.store_policy_for(build_config(GUST, n), "auto") == auto_policy(n), n
    assert auto_policy(edge) != auto_policy(edge + 1) == (NT, NT, PLAIN)
    for text in COMPILED:
        assert native.store_policy_for(build_config(GUST, 300), text) == auto_policy(300)
        assert native.store_policy_for(build_config(GUST, SMALL_N_MAX), text) == auto_policy(SMALL_N_MAX)
    # another configuration moves other bytes per env-step: the boundary moves with them
    sb = step_bytes(build_config(SIMPLE, 4))
    assert step_bytes(build_config(GUST, 4)) == BENCH_STEP_BYTES != sb
    e2 = NT_STATE_BYTES // sb
    assert e2 != edge
    assert native.store_policy_for(build_config(SIMPLE, e2), "auto") == (WT, NT_WT, PLAIN)
    assert native.store_policy_for(build_config(SIMPLE, e2 + 1), "auto") == (NT, NT, PLAIN)


# ---- on the GPU ----
def _env(env_id, n, policy, **kw):
    from cf2sim.vec_env import BatchedCrazyflieEnv
    old = os.environ.get("CF2SIM_STORE_POLICY")
    os.environ["CF2SIM_STORE_POLICY"] = policy
    try:
        return BatchedCrazyflieEnv(env_id, n, seed=3, want_final_obs=True, **kw)
    finally:
        if old is None:
            del os.environ["CF2SIM_STORE_POLICY"]
        else:
            os.environ["CF2SIM_STORE_POLICY"] = old


def _actions(n, steps):
    rng = np.random.default_rng(17)
    return torch.from_numpy(np.stack([wide_actions(rng, n) for _ in range(steps)])).cuda()


def _steps(env_id, n, policy, acts, **kw):
    """Every output of every env-step, and the snapshot after the last one."""
    e = _env(env_id, n, policy, **kw)
    out = {"obs0": e.reset().clone()}
    rec = {k: [] for k in ("obs", "rew", "done", "trunc", "cost", "level", "final_obs")}
    for a in acts:
        o, r, d, info = e.step(a)
        for k, v in (("obs", o), ("rew", r), ("done", d), ("trunc", info["truncated"]), ("cost", info["cost"]),
                     ("level", info["disturbance_level"]), ("final_obs", info["final_obs"])):
            rec[k].append(v.clone())
    out.update({k: torch.stack(v) for k, v in rec.items()})
    out["state_f"], out["state_i"] = e.get_state()
    e.check_device_errors()
    out["policy"] = e.store_policy
    e.close()
    return out


def _assert_same(got, ref, what):
    for k, r in ref.items():
        if k == "policy":
            continue
        # bit patterns: NaNs and signed zeros count
        g = got[k]
        same = torch.equal(g.view(torch.int32), r.view(torch.int32)) if g.dtype == torch.float32 else torch.equal(g, r)
        assert same, f"{what}: {k} differs from the plain policy's"


STEP_CASES = {
    # whole blocks time out together: every block runs reset chunks
    "gust_timeout7": (GUST, N1, dict(max_episode_steps=7)),
    # default TimeLimit: resets come from crashes at random lanes next to lanes that do not reset
    "gust_crashes": (GUST, N1, {}),
    # a generic (SPEC 0) instance
    "simple_generic": (SIMPLE, N1, dict(max_episode_steps=9)),
}
_plain = {}


def _plain_steps(case):
    if case not in _plain:
        env_id, n, kw = STEP_CASES[case]
        _plain[case] = (_steps(env_id, n, "plain", _actions(n, 40), **kw), _actions(n, 40))
    return _plain[case]


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [p for p in COMPILED if p != "plain"])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_kernel_results_do_not_depend_on_the_policy(gpu, case, policy):
    env_id, n, kw = STEP_CASES[case]
    ref, acts = _plain_steps(case)
    assert ref["policy"] == COMPILED["plain"]
    assert ref["done"].any() and not ref["done"].all(), "the run needs resets next to envs that go on"
    if case == "gust_crashes":
        assert ref["done"].sum() > ref["trunc"].sum(), "no crash resets in the window"
    got = _steps(env_id, n, policy, acts, **kw)
    assert got["policy"] == COMPILED[policy]
    _assert_same(got, ref, f"{case} under {policy}")


@pytest.mark.gpu
def test_getter_reports_what_runs(gpu, native):
    for text, pol in COMPILED.items():
        e = _env(GUST, N1, text)
        assert e.store_policy == pol == native.store_policy_for(build_config(GUST, N1), text)
        e.close()
    for n in (300, N1):
        e = _env(GUST, n, "auto")
        assert e.store_policy == auto_policy(n)
        e.close()
    # 1 Mi envs: config arithmetic only, nothing is allocated
    assert native.store_policy_for(build_config(GUST, 1 << 20), "auto") == auto_policy(1 << 20) == (NT, NT, PLAIN)
    old = os.environ.get("CF2SIM_STORE_POLICY")
    os.environ["CF2SIM_STORE_POLICY"] = "sc1"
    try:
        from cf2sim.vec_env import BatchedCrazyflieEnv
        with pytest.raises(native.CF2Error, match="invalid argument"):
            BatchedCrazyflieEnv(GUST, N1)
    finally:
        if old is None:
            del os.environ["CF2SIM_STORE_POLICY"]
        else:
            os.environ["CF2SIM_STORE_POLICY"] = old
