"""cf2_set_level_distribution / BatchedCrazyflieEnv.set_level_distribution: the per-episode
disturbance level is drawn from the caller's weights from the next reset on.  The reference fixes
the weights to Boltzmann() (envs/utils.py:27-39) and registers "...WithCurriculumHJAdversary" with
that same distribution; this is the hook a curriculum needs."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
from parity_util import copy_config

pytestmark = pytest.mark.gpu

ENV = "DroneHoverBulletFreeEnvWithCurriculumHJAdversary-v0"
N = 4096


@functools.lru_cache(maxsize=None)
def _table():
    return torch.from_numpy((np.linspace(-1, 1, 15 ** 6, dtype=np.float32) ** 3).reshape(1, -1)).cuda()


def _env(n=N, **kw):
    from cf2sim.vec_env import BatchedCrazyflieEnv
    e = BatchedCrazyflieEnv(ENV, n, seed=3, max_episode_steps=3, **kw)
    e.bind_hj_tables(_table(), [0] * int(e.cfg.num_levels))
    return e


def _levels_after_reset(e, generations=3, reset=True):
    """Levels reported by the 3 * generations + 1 steps after a reset, [steps, N] on the host.
    max_episode_steps = 3: every episode lasts at most three steps (some envs crash sooner), so every
    env has begun its episodes 0 .. generations by the last step."""
    if reset:
        e.reset()
    act = torch.zeros(e.num_envs, 4, device=e.device)
    out, dones = [], []
    for _ in range(3 * generations + 1):
        _, _, done, info = e.step(act)
        out.append(info["disturbance_level"].clone())
        dones.append(done.clone())
    torch.cuda.synchronize()
    levels, dones = torch.stack(out).cpu().numpy(), torch.stack(dones).cpu().numpy().astype(bool)
    assert dones.any() and (levels[1:] == levels[:-1])[~dones[:-1]].all(), "a level changes only at an episode's end"
    _levels_after_reset.dones = dones
    return levels


def _episode_levels(levels, dones, g):
    """The level of every env's g-th episode since the reset ([N]): each is one draw from the
    distribution, whenever the episode began."""
    ep = np.concatenate([np.zeros((1, dones.shape[1]), np.int64), np.cumsum(dones, axis=0)[:-1]])
    assert (ep == g).any(axis=0).all(), f"not every env has begun episode {g}"
    return levels[(ep == g).argmax(axis=0), np.arange(dones.shape[1])]


def _one_hot(k, L=21):
    p = [0.0] * L
    p[k] = 1.0
    return p


@pytest.mark.parametrize("k", [7, 0, 20])
def test_one_hot_distribution(gpu, k):
    e = _env()
    lv = np.array([e.cfg.level_values[j] for j in range(21)], dtype=np.float32)
    before = _levels_after_reset(e, 1)
    assert np.unique(before).size > 5, "the default Boltzmann() weights draw many levels"
    e.set_level_distribution(_one_hot(k))
    got = _levels_after_reset(e)
    assert got.shape == (10, N) and (got.view(np.uint32) == lv[k].view(np.uint32)).all(), np.unique(got)
    e.close()


def test_two_level_distribution_counts_and_oracle(gpu):
    e = _env()
    L = int(e.cfg.num_levels)
    lv = np.array([e.cfg.level_values[j] for j in range(L)], dtype=np.float32)
    p = [0.0] * L
    p[2] = p[9] = 0.5
    e.set_level_distribution(p)
    e.reset()
    idx = e.get_state()[1][e.layout.i_level].cpu().numpy()
    # the CPU restatement with the same CDF draws the same level for every env
    ref = O.OracleEnv(copy_config(e.cfg), precision="f32")
    ref.reset()
    assert np.array_equal(ref.get_state()[1][e.layout.i_level], idx)
    ref.close()
    got = _levels_after_reset(e, reset=False)
    assert np.array_equal(lv[idx].view(np.uint32), got[0].view(np.uint32)), "the first step reports the reset's level"
    assert set(np.unique(got).tolist()) == {float(lv[2]), float(lv[9])}
    # Binomial(4096, 1/2): sigma = 32, 5 sigma = 160; the distribution itself leaves this with p < 1e-6
    dones = _levels_after_reset.dones
    gens = [_episode_levels(got, dones, g) for g in range(4)]      # after the reset and after three auto-resets
    for row in gens:
        assert abs(int((row == lv[2]).sum()) - N // 2) <= 160, int((row == lv[2]).sum())
    assert np.array_equal(gens[0], got[0]) and not np.array_equal(gens[0], gens[3]), "levels are redrawn at an auto-reset"
    e.close()


def test_running_episodes_keep_their_level(gpu):
    e = _env()
    e.reset()
    act = torch.zeros(N, 4, device=gpu)
    first = e.step(act)[3]["disturbance_level"].clone()
    done1 = e.done.clone().bool()
    e.set_level_distribution(_one_hot(20))
    info = e.step(act)[3]
    torch.cuda.synchronize()
    second = info["disturbance_level"]
    assert torch.equal(second[~done1], first[~done1]), "an episode under way keeps its level"
    assert done1.sum() == 0 or (second[done1] == 2.0).all(), "an env that reset after the call draws from the new weights"
    for _ in range(3):
        e.step(act)
    assert (e.step(act)[3]["disturbance_level"] == 2.0).all(), "after every env has reset, every level is the new one"
    e.close()


def test_split_contexts_draw_the_same_levels(gpu):
    p = np.linspace(0.0, 1.0, 21) ** 2                      # unnormalised, level 0 never drawn
    whole = _env()
    parts = [_env(N // 2, env_id_offset=k * (N // 2)) for k in range(2)]
    for e in [whole] + parts:
        e.set_level_distribution(p)
    a = _levels_after_reset(whole)
    b = np.concatenate([_levels_after_reset(e) for e in parts], axis=1)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (a != 0.0).all() and np.unique(a).size > 10
    for e in [whole] + parts:
        e.close()


def test_rejected_distributions(gpu):
    from cf2sim import _native
    from cf2sim.vec_env import BatchedCrazyflieEnv
    e = _env(64)
    cdf = [float(e.cfg.level_cdf[k]) for k in range(21)]
    for bad in ([1.0] * 20, [1.0] * 22, [0.0] * 21, [1.0] * 20 + [-1.0], [1.0] * 20 + [float("nan")],
                [1.0] * 20 + [float("inf")]):
        with pytest.raises(_native.CF2Error):
            e.set_level_distribution(bad)
        assert [float(e.cfg.level_cdf[k]) for k in range(21)] == cdf, "a rejected call changes nothing"
    assert e.lib.cf2_set_level_distribution(e._ctx, None, 21) == _native.CF2_ERR_INVALID_ARG
    e.close()
    fixed = BatchedCrazyflieEnv("DroneHoverBulletFreeEnvWithGust-v0", 64)
    with pytest.raises(_native.CF2Error, match="status -4"):
        fixed.set_level_distribution([1.0] * int(fixed.cfg.num_levels))
    fixed.close()


def test_device_error_word_survives(gpu):
    """Only the CDF's words of the device tables are uploaded: setting a distribution reports no device
    error and clears none (cf2_device_errors still reads 0, the env steps on)."""
    e = _env(64)
    e.set_level_distribution(_one_hot(4))
    e.check_device_errors()
    got = _levels_after_reset(e, 1)
    assert (got == np.float32(e.cfg.level_values[4])).all()
    e.check_device_errors()
    e.close()


def test_checkpoint_keeps_the_distribution(gpu, tmp_path):
    from cf2sim.config import level_cdf_from
    from cf2sim.vec_env import BatchedCrazyflieEnv
    e = _env(512)
    p = [0.0] * 21
    p[5], p[6], p[17] = 1.0, 2.0, 1.0
    e.set_level_distribution(p)
    assert [float(e.cfg.level_cdf[k]) for k in range(21)] == level_cdf_from(p)
    e.reset()
    path = str(tmp_path / "ckpt.safetensors")
    e.save_checkpoint(path)
    r = BatchedCrazyflieEnv.from_checkpoint(path)
    r.bind_hj_tables(_table(), [0] * 21)
    assert bytes(r.cfg) == bytes(e.cfg) and [float(r.cfg.level_cdf[k]) for k in range(21)] == level_cdf_from(p)
    act = torch.zeros(512, 4, device=gpu)
    allowed = torch.tensor([e.cfg.level_values[k] for k in (5, 6, 17)], dtype=torch.float32, device=gpu)
    for _ in range(10):                                     # both resume bit-identically, auto-resets included
        a, b = e.step(act), r.step(act)
        assert torch.equal(a[0], b[0]) and torch.equal(a[3]["disturbance_level"], b[3]["disturbance_level"])
        assert torch.isin(b[3]["disturbance_level"], allowed).all()
    assert torch.unique(b[3]["disturbance_level"]).numel() == 3
    e.close()
    r.close()
