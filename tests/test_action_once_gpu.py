"""The latency ring's compact form and the gust torque's store on change (DESIGN.md section 3,
"Bytes the result does not need").

Where an env-step writes the whole latency ring (latency on, aggregate_phy_steps >= ring rows), it
stores the step's action once, in ring row 0, and marks the env compact in its flag word; ring rows
r >= 1 and action_history[1] are then stale in memory and every reader takes them from row 0.  In
gust mode the torque group is stored only in lanes where it changed.

Reference of every case: a second env of the same configuration whose state goes through get_state /
set_state before every call.  An import writes explicit rows and a clear flag, so that env always runs
the path the kernels had before the compact form existed.  Every output of every call and the exported
state after it must be bit-identical between the two.  The stale slots hold older values than the true
ones (the ring rows of the last reset or import, not the last action), so this comparison is also what
shows that nothing reads them.

Not tested: overwriting the stale slots themselves with NaN.  The library has no route to them that
keeps the flag: cf2_set_state writes explicit rows and clears it, and no debug hook was added for it.
"""
import ctypes

import numpy as np
import pytest
import torch

from parity_util import N1, SMALL_N_MAX, wide_actions

GUST = "DroneHoverBulletFreeEnvWithGust-v0"
N_SMALL = 321                     # small-N kernel: five full blocks of 64 envs and one lane
OUTPUTS = ("obs", "rew", "done", "trunc", "cost", "level", "final_obs")


def _same(a, b):
    """Bit patterns: NaNs and signed zeros count."""
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _actions(n, steps, seed=17):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([wide_actions(rng, n) for _ in range(steps)])).cuda()


class Pair:
    """The env under test and its reference, which is re-imported before every call."""

    def __init__(self, n, **kw):
        from cf2sim.vec_env import BatchedCrazyflieEnv
        self.n = n
        self.env = BatchedCrazyflieEnv(GUST, n, seed=3, want_final_obs=True, **kw)
        self.ref = BatchedCrazyflieEnv(GUST, n, seed=3, want_final_obs=True, **kw)
        self.calls = 0
        self.done = torch.zeros(n, dtype=torch.bool, device="cuda")
        assert _same(self.env.reset(), self.ref.reset())
        self.check_state("reset")

    def reimport(self):
        sf, si = self.ref.get_state()
        self.ref.set_state(sf, si)

    def check_state(self, what):
        (ef, ei), (rf, ri) = self.env.get_state(), self.ref.get_state()
        L = self.env.layout
        if not _same(ef, rf):
            rows = sorted(set(torch.nonzero(ef.view(torch.int32) != rf.view(torch.int32))[:, 0].tolist()))
            raise AssertionError(f"{what}: exported float fields {rows} differ (f_abuf {L.f_abuf}, f_hist_act "
                                 f"{L.f_hist_act}, f_dstb {L.f_dstb})")
        assert _same(ei, ri), f"{what}: exported int fields differ"
        assert int((ei[L.i_flags] >> 8).max()) == 0, f"{what}: an exported flag word has bits past 7"
        return ef, ei

    def step(self, a):
        self.reimport()
        what = f"call {self.calls} (step)"
        eo, er, ed, ei = self.env.step(a)
        ro, rr, rd, ri = self.ref.step(a)
        got = dict(obs=eo, rew=er, done=ed, trunc=ei["truncated"], cost=ei["cost"], level=ei["disturbance_level"],
                   final_obs=ei["final_obs"])
        ref = dict(obs=ro, rew=rr, done=rd, trunc=ri["truncated"], cost=ri["cost"], level=ri["disturbance_level"],
                   final_obs=ri["final_obs"])
        for k in OUTPUTS:
            assert _same(got[k], ref[k]), f"{what}: {k} differs"
        self.last_done = ed.bool().clone()
        self.done |= self.last_done
        self.calls += 1
        return self.check_state(what)

    def close(self):
        for e in (self.env, self.ref):
            e.check_device_errors()
            e.close()


def _run(n, steps, **kw):
    p = Pair(n, **kw)
    for a in _actions(n, steps):
        p.step(a)
    done = p.done.clone()
    p.close()
    return done


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N1, N_SMALL])
def test_default_episodes_mix_fresh_and_compact_lanes(gpu, n):
    """Default kwargs: crashes reset single lanes (explicit rows, clear flag) next to compact ones."""
    assert N_SMALL <= SMALL_N_MAX < N1
    done = _run(n, 40)
    assert not done.all()
    if n == N1:
        assert done.any(), "the run needs resets next to envs that go on"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N1, N_SMALL])
def test_whole_blocks_reset_in_one_step(gpu, n):
    done = _run(n, 40, max_episode_steps=7)
    assert done.all()


@pytest.mark.gpu
def test_fused_rollout_from_compact_state(gpu):
    """3 single steps (the state is compact), one fused launch of K = 8, 2 single steps, against 13
    single steps of the re-imported reference."""
    K = 8
    p = Pair(N1, max_episode_steps=7)
    acts = _actions(N1, 3 + K + 2)
    for a in acts[:3]:
        p.step(a)
    obs, rew, done, info = p.env.rollout(acts[3:3 + K].contiguous())
    for k in range(K):
        p.reimport()
        ro, rr, rd, ri = p.ref.step(acts[3 + k])
        what = f"rollout step {k}"
        assert _same(obs[k], ro), f"{what}: obs differs"
        assert _same(rew[k], rr), f"{what}: rew differs"
        assert _same(done[k], rd), f"{what}: done differs"
        assert _same(info["truncated"][k], ri["truncated"]), f"{what}: trunc differs"
        assert _same(info["cost"][k], ri["cost"]), f"{what}: cost differs"
        assert _same(info["disturbance_level"][k], ri["disturbance_level"]), f"{what}: level differs"
        assert _same(info["final_obs"][k][rd.bool()], ri["final_obs"][rd.bool()]), f"{what}: final_obs differs"
    p.check_state("after the rollout")
    # the single-step outputs' final_obs rows are only written for envs that finish: align the buffers
    p.env.final_obs.copy_(p.ref.final_obs)
    for a in acts[3 + K:]:
        p.step(a)
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N1, N_SMALL])
@pytest.mark.parametrize("shape", ["ring4", "agg1", "agg4"])
def test_other_shapes(gpu, n, shape):
    """ring4 (latency 0.02: four rows, two sub-steps) and agg1 (one sub-step, two rows) must never go
    compact: the action must not leak into rows the step did not write.  agg4 is a generic-shape
    instance whose four sub-steps do write both rows: it goes compact."""
    kw = {"ring4": dict(latency=0.02), "agg1": dict(aggregate_phy_steps=1), "agg4": dict(aggregate_phy_steps=4)}[shape]
    p = Pair(n, max_episode_steps=9, **kw)
    c = p.env.cfg
    assert (int(c.aggregate_phy_steps), int(c.buf_size)) == {"ring4": (2, 4), "agg1": (1, 2), "agg4": (4, 2)}[shape]
    L = p.env.layout
    for a in _actions(n, 12):
        sf, _ = p.step(a)
        # (an env that reset in this step holds the reset's ring, whose rows are drawn one by one)
        ring = sf[L.f_abuf:L.f_abuf + 4 * int(c.buf_size)].view(int(c.buf_size), 4, n)[:, :, ~p.last_done]
        equal_rows = bool((ring == ring[0]).all())
        if shape == "agg4":
            assert equal_rows, "four sub-steps write both rows"
    if shape != "agg4":
        assert not equal_rows, "a ring longer than the sub-steps keeps older actions"
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N1, N_SMALL])
def test_gust_torque_across_onsets_and_expiries(gpu, n):
    p = Pair(n, gust_onset_prob=0.2, gust_duration=3)
    L = p.env.layout
    on_prev = None
    onsets = expiries = 0
    for a in _actions(n, 40):
        sf, si = p.step(a)            # the exported dstb is part of the compared state
        on = (sf[L.f_dstb:L.f_dstb + 3] != 0).any(0)
        if on_prev is not None:
            onsets += int((on & ~on_prev).sum())
            expiries += int((~on & on_prev).sum())
        on_prev = on
    assert onsets > n and expiries > n, (onsets, expiries)
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N1, N_SMALL])
def test_physics_substep_and_masked_reset_between_steps(gpu, n):
    p = Pair(n, max_episode_steps=9)
    acts = _actions(n, 10)
    for a in acts[:3]:
        p.step(a)
    # one physics plug-in sub-step on the compact state: the rows are unequal afterwards
    for e in (p.ref, p.env):
        if e is p.ref:
            p.reimport()
        st = e.lib.cf2_physics_step(e._ctx, acts[3].data_ptr(), None, ctypes.c_float(0.0), e.stream)
        assert st == 0
    sf, _ = p.check_state("physics sub-step")
    L = p.env.layout
    assert not bool((sf[L.f_abuf:L.f_abuf + 4] == sf[L.f_abuf + 4:L.f_abuf + 8]).all())
    for a in acts[4:7]:
        p.step(a)
    # a masked reset of every third env, then env-steps
    mask = (torch.arange(n, device="cuda") % 3 == 0)
    p.reimport()
    assert _same(p.env.reset(mask), p.ref.reset(mask))
    p.check_state("masked reset")
    for a in acts[7:]:
        p.step(a)
    p.close()
