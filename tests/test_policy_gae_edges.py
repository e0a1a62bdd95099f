"""cf2_policy_forward, cf2_value_forward_masked and cf2_gae (csrc/cf2sim_policy.hip) against float64
references at the sizes where the kernels take the paths a collect at workload size runs: several
chunks per wave of the persistent policy grid (the observation prefetch, the per-lane constants
re-used across chunks, the shared sampling noise with its ds_bpermute routing and its redraw at
the fifth chunk), the masked value pass's per-block early exit, and the GAE scan's 8-step load
block at T below, at and above a multiple of 8 with the reward clip active.

References.  Policy: ``copy.deepcopy(ac).double()`` on the device, every row, mixed error
|g - r| / (1 + |r|) held to test_rollout.POLICY_TOL per trip ``kk`` of the chunk loop.  Noise: a
numpy Philox4x32-10 + float64 Box-Muller (checked against oracle.philox without a GPU), every row
and all four components, eps recovered as (act - mu_det) / std with the kernel's own deterministic
mu, so the network error cancels.  GAE: ``cf2sim.rollout.gae`` in float64, every env; per output
tensor |g - g64|_inf / |g64|_inf of the kernel is at most 8 x that of ``gae`` in torch float32 on
the same inputs, floor 2^-20 (the rule of tests/test_ppo_update.py).

Measured on an MI355X (256 CUs, n = 294 919 rows: trips kk = 0..4; the full table is
profiles/policy_gae_parity.txt):

    worst over kk = 0..4     mu D=34    mu D=42    V D=34     V D=42     bound (POLICY_TOL)
    fp32                     6.3e-7     2.1e-6     2.2e-7     3.6e-7     2e-5
    bf16x3                   3.7e-5     8.4e-5     9.5e-6     6.4e-6     1.5e-4
    (the five trips agree within a factor 1.4: no trip is worse than the first)
    noise, all rows x 4      2.1e-6 absolute (bound 2e-4: the worst is 1 % of it, so the bound of
                             tests/test_rollout.py stands); logp 3.9e-7 mixed (bound 1e-4)
    mode 1 vs mode 0         marked rows bit-equal in all 7 mask patterns, D and precisions
    GAE, 30 shapes x 3       kernel <= 3.0e-7, torch fp32 <= 3.8e-7 (|.|_inf relative, adv / ret /
                             disc): below the floor 2^-20 = 9.5e-7, the 8 x allowance is not needed

Mutations (scratch builds, never committed; profiles/policy_gae_parity.txt has the table): the noise
source lane from kk & 1, the redraw every 8th chunk, the prefetch of chunk c + nwaves + 1, mode 1's
per_block without PW, GAE without the reset at done, and a clip bound of 1 each fail tests here.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from test_rollout import POLICY_TOL

MASK32 = np.uint64(0xFFFFFFFF)
NOISE_TOL = 2e-4          # absolute, on eps; test_rollout.py's bound (measured worst: see the docstring)
LOGP_TOL = 1e-4           # mixed, as test_rollout.py
FLOOR = 2.0 ** -20
SEED = (0x9E3779B9 << 32) | 1234      # both key words in use
DIMS_PRECS = [(34, "fp32"), (34, "bf16x3"), (42, "fp32"), (42, "bf16x3")]
LOG_STD = [math.log(0.5), math.log(0.3), math.log(0.9), math.log(0.15)]


# ---------------------------------------------------------------- helpers (no GPU)
def philox4x32_10(ctr, key):
    """Philox4x32-10 over arrays: ctr = 4 and key = 2 integer arrays (broadcast against each other),
    values taken mod 2^32.  uint64 products, the halves and the key schedule wrapped to 32 bits as
    csrc/cf2sim_rng.h does.  Returns 4 uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & MASK32 for c in ctr])
    k0, k1 = [np.asarray(k, dtype=np.uint64) & MASK32 for k in key]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s = np.uint64(32)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & MASK32
            k1 = (k1 + np.uint64(0xBB67AE85)) & MASK32
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & MASK32, (p0 >> s) ^ c3 ^ k1, p0 & MASK32
    return c0, c1, c2, c3


def box_muller64(a, b):
    """The kernel's Box-Muller pair in float64: u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24."""
    u1 = ((a >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (b >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def policy_normals(seed, counter, row_offset, rows):
    """[len(rows), 4] float64: the sampling noise cf2_policy_forward gives rows `rows` of a call with
    this seed, call counter and row_offset: Philox counter [0, counter, (row_offset + row) mod 2^32, 3]
    (TAG_POLICY), key (seed lo, seed hi), two Box-Muller pairs."""
    prow = (np.asarray(rows, dtype=np.uint64) + np.uint64(row_offset)) & MASK32
    u = philox4x32_10([0, counter, prow, 3], [seed & 0xFFFFFFFF, seed >> 32])
    z0, z1 = box_muller64(u[0], u[1])
    z2, z3 = box_muller64(u[2], u[3])
    return np.stack([z0, z1, z2, z3], axis=1)


def policy_geometry(n, cus):
    """Which wave runs which rows in which trip of its chunk loop.  Mirrors policy_grid() and the
    chunk loop of policy_kernel in csrc/cf2sim_policy.hip (which carries the matching comment): a
    change there must be made here too.  Blocks of 8 waves, at most 2 per CU, 16-row chunks; wave
    w runs chunks w, w + nwaves, ...; kk counts a wave's trips."""
    blocks = min(-(-n // 128), 2 * cus)
    nwaves = 8 * blocks
    chunk = np.arange(n, dtype=np.int64) // 16
    wave = chunk % nwaves
    return {"n": n, "blocks": blocks, "nwaves": nwaves, "nchunks": -(-n // 16), "chunk": chunk, "wave": wave,
            "block": wave // 8, "kk": chunk // nwaves}


def edge_rows(cus):
    """A row count at which a full grid's waves run 4 chunks and half of them a fifth, the last
    chunk ragged (7 rows): 294 919 at 256 CUs."""
    nwaves = 8 * 2 * cus
    return 16 * (4 * nwaves + nwaves // 2) + 7


def check_coverage(geo):
    """The conditions that keep the large tests from shrinking to one chunk per wave."""
    kk = geo["kk"]
    assert kk.max() == 4, f"kk reaches {kk.max()}, not 4"
    counts = np.bincount(kk, minlength=5)
    assert (counts >= 1000).all(), f"rows per kk class {counts.tolist()}"
    return counts


def test_numpy_philox_equals_oracle():
    import oracle as O
    rng = np.random.default_rng(11)
    m = 1200
    ctr = rng.integers(0, 2 ** 32, size=(m, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(m, 2), dtype=np.uint64)
    ctr[:8] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0, 1, 0xFFFFFFFF, 3], [0, 0xFFFFFFFF, 0, 3],
               [0xFFFFFFFF, 0, 0, 0], [0, 0, 0xFFFFFFFF, 0], [1, 2, 3, 4], [0, 5, 2 ** 31, 3]]
    key[:4] = [[0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 0], [0, 0xFFFFFFFF]]
    got = np.stack(philox4x32_10([ctr[:, i] for i in range(4)], [key[:, 0], key[:, 1]]), axis=1)
    want = np.array([O.philox(ctr[i].tolist(), key[i].tolist()) for i in range(m)], dtype=np.uint64)
    assert np.array_equal(got, want)
    # rows that wrap 2^32: row_offset + row is taken mod 2^32, as the kernel's uint32 sum
    off, rows = 2 ** 32 - 100, np.array([0, 1, 99, 100, 101, 2999])
    z = policy_normals(SEED, 0xFFFFFFFF, off, rows)
    for i, r in enumerate(rows):
        u = O.philox([0, 0xFFFFFFFF, (off + int(r)) % 2 ** 32, 3], [SEED & 0xFFFFFFFF, SEED >> 32])
        for pair in (0, 1):
            u1 = ((u[2 * pair] >> 8) + 1.0) * 2.0 ** -24
            u2 = (u[2 * pair + 1] >> 8) * 2.0 ** -24
            rad = math.sqrt(-2.0 * math.log(u1))
            want = [rad * math.cos(2 * math.pi * u2), rad * math.sin(2 * math.pi * u2)]
            np.testing.assert_allclose(z[i, 2 * pair:2 * pair + 2], want, rtol=0, atol=1e-14)
    np.testing.assert_array_equal(policy_normals(SEED, 7, off, [100, 101]), policy_normals(SEED, 7, 0, [0, 1]))
    # the normals are standard: mean 0, variance 1 over 2 * 10^5 draws (5 sigma of the estimators)
    z = policy_normals(SEED, 3, 0, np.arange(50_000))
    assert abs(z.mean()) < 5 / math.sqrt(z.size) and abs(z.var() - 1.0) < 5 * math.sqrt(2.0 / z.size)


def test_policy_geometry_at_256_cus():
    n = edge_rows(256)
    assert n == 294_919
    geo = policy_geometry(n, 256)
    assert geo["blocks"] == 512 and geo["nwaves"] == 4096 and geo["nchunks"] == 18_433
    counts = check_coverage(geo)
    assert counts.tolist() == [65_536] * 4 + [2048 * 16 + 7]
    assert np.count_nonzero(geo["chunk"] == geo["nchunks"] - 1) == 7             # ragged last chunk
    fifth = np.unique(geo["wave"][geo["kk"] == 4])
    assert fifth.tolist() == list(range(2049))                                   # half the waves (+ the ragged one)
    # the kk = 4 redraw: lane groups 1..3 would draw chunks c + g nwaves, all past nchunks
    first = geo["chunk"][geo["kk"] == 4].min()
    assert first == 4 * geo["nwaves"] and first + geo["nwaves"] >= geo["nchunks"]
    # a grid that is not full: every wave has one chunk at most
    small = policy_geometry(3000, 256)
    assert small["blocks"] == 24 and small["kk"].max() == 0
    assert policy_geometry(1, 256)["nwaves"] == 8 and policy_geometry(129, 256)["blocks"] == 2


# ---------------------------------------------------------------- policy forward (GPU)
def mixed_err(g, r):
    """per row max over components of |g - r| / (1 + |r|), float64"""
    e = (g.double() - r).abs() / (1.0 + r.abs())
    return e if e.dim() == 1 else e.amax(dim=1)


@functools.lru_cache(maxsize=None)
def network(gpu, d, precision):
    """The networks of test_fused_policy_matches_torch_networks (same seed: random biases, observation
    statistics away from identity, feature std down to ~0.05) with four different log_std, the
    fused wrapper and the float64 copy."""
    from cf2sim.rollout import FusedActorCritic, MLPActorCritic
    torch.manual_seed(d)
    ac = MLPActorCritic(obs_dim=d).to(gpu)
    for m in ac.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.uniform_(m.bias, -0.3, 0.3)
    ac.obs_oms.update(torch.randn(5000, d, device=gpu) * torch.rand(d, device=gpu) * 4 + 1.0)
    with torch.no_grad():
        ac.log_std.copy_(torch.tensor(LOG_STD, device=gpu))
    return ac, FusedActorCritic(ac, seed=SEED, precision=precision), copy.deepcopy(ac).double()


def reference64(ac64, obs):
    with torch.no_grad():
        x = ac64.normalize(obs.double())
        return ac64.pi_net(x), ac64.v_net(x).squeeze(-1)


COUNTER = 5      # the call counter of the sampled steps below


def sampled(fused, obs, counter=COUNTER, row_offset=0):
    fused.counter = counter
    return fused.step(obs, row_offset=row_offset)


@functools.lru_cache(maxsize=None)
def big_case(gpu, d, precision):
    """One deterministic and one sampled launch at the edge row count, with the float64 reference:
    computed once per (D, precision), shared by the tests below, never modified."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = edge_rows(cus)
    geo = policy_geometry(n, cus)
    check_coverage(geo)
    ac, fused, ac64 = network(gpu, d, precision)
    g = torch.Generator(device=gpu).manual_seed(1000 + d)
    obs = torch.randn(n, d, device=gpu, generator=g) * 3
    mu_ref, v_ref = reference64(ac64, obs)
    a_det, v_det, lp_det = fused.step(obs, deterministic=True)
    act, val, logp = sampled(fused, obs)
    return {"n": n, "geo": geo, "kk": torch.as_tensor(geo["kk"], device=gpu), "obs": obs, "mu_ref": mu_ref,
            "v_ref": v_ref, "a_det": a_det, "v_det": v_det, "lp_det": lp_det, "act": act, "val": val, "logp": logp}


def check_noise(tag, act, a_det, logp, log_std64, normals):
    """eps = (act - mu_det) / std against the float64 normals, every row and component; logp against
    sum(-eps^2 / 2 - log_std - log(2 pi) / 2) of those normals.  Returns the worst errors."""
    z = torch.as_tensor(normals, device=act.device)
    eps = (act.double() - a_det.double()) / log_std64.exp()
    e_eps = (eps - z).abs()
    worst = float(e_eps.max())
    lp_ref = (-0.5 * z * z - log_std64 - 0.5 * math.log(2 * math.pi)).sum(-1)
    e_lp = float(mixed_err(logp, lp_ref).max())
    print(f"PARITY noise {tag}: eps worst {worst:.3e} (row {int(e_eps.amax(dim=1).argmax())}), logp worst {e_lp:.3e}")
    assert worst < NOISE_TOL, f"{tag}: noise differs by {worst:.3e} at row {int(e_eps.amax(dim=1).argmax())}"
    assert e_lp < LOGP_TOL, f"{tag}: logp differs by {e_lp:.3e}"
    return worst, e_lp


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dim,precision", DIMS_PRECS)
def test_policy_mu_and_value_per_trip(gpu, obs_dim, precision):
    """mu and V of every row of a launch whose waves run up to 5 chunks, per trip kk."""
    B = big_case(gpu, obs_dim, precision)
    e_mu, e_v = mixed_err(B["a_det"], B["mu_ref"]), mixed_err(B["v_det"], B["v_ref"])
    assert torch.equal(B["lp_det"], torch.ones_like(B["lp_det"]))      # deterministic: logp = 1, as the module
    assert torch.equal(B["val"], B["v_det"])                           # the value does not depend on sampling
    bad = []
    for k in range(5):
        sel = B["kk"] == k
        m, v = float(e_mu[sel].max()), float(e_v[sel].max())
        print(f"PARITY policy D={obs_dim} {precision} kk={k} rows={int(sel.sum())}: mu {m:.3e} V {v:.3e}")
        if not (m < POLICY_TOL[precision] and v < POLICY_TOL[precision]):
            bad.append(f"kk={k}: mu {m:.3e} V {v:.3e}")
    assert not bad, f"D={obs_dim} {precision}, bound {POLICY_TOL[precision]}: " + "; ".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dim,precision", DIMS_PRECS)
def test_policy_noise_and_logp_every_row(gpu, obs_dim, precision):
    """The sampling noise of all rows and components is Philox(seed, counter, row): the rows of
    trips kk & 3 = 1..3 take theirs from lane groups 1..3, trip 4 from the redraw."""
    B = big_case(gpu, obs_dim, precision)
    ac64 = network(gpu, obs_dim, precision)[2]
    z = policy_normals(SEED, COUNTER, 0, np.arange(B["n"]))
    zt = torch.as_tensor(z, device=gpu)
    eps = (B["act"].double() - B["a_det"].double()) / ac64.log_std.exp()
    per_kk = [float((eps - zt).abs()[B["kk"] == k].max()) for k in range(5)]
    print(f"PARITY noise D={obs_dim} {precision} per kk: " + " ".join(f"{e:.3e}" for e in per_kk))
    wrong = [k for k in range(5) if not per_kk[k] < NOISE_TOL]
    assert not wrong, f"noise of trips kk={wrong} differs: {per_kk}"
    check_noise(f"D={obs_dim} {precision} n={B['n']}", B["act"], B["a_det"], B["logp"], ac64.log_std, z)


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dim,precision", DIMS_PRECS)
def test_policy_is_invariant_to_launch_geometry(gpu, obs_dim, precision):
    """Bitwise: the rows as slices of 4096 (one chunk per wave, row_offset = slice start, the same
    counter) equal the big launch's act, val and logp."""
    B = big_case(gpu, obs_dim, precision)
    fused = network(gpu, obs_dim, precision)[1]
    for s in range(0, B["n"], 4096):
        e = min(s + 4096, B["n"])
        a, v, lp = sampled(fused, B["obs"][s:e], row_offset=s)
        for name, got, want in (("act", a, B["act"]), ("val", v, B["val"]), ("logp", lp, B["logp"])):
            assert torch.equal(got, want[s:e]), f"{name} of rows {s}..{e} depends on the launch geometry"


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_policy_row_offset_wraps(gpu, precision):
    """row_offset + row is a uint32 sum: a launch at row_offset 2^32 - 100 gives rows 100.. the
    noise of global rows 0.., and equals the two launches split at the wrap bit for bit."""
    ac, fused, ac64 = network(gpu, 34, precision)
    n, off = 3000, 2 ** 32 - 100
    obs = torch.randn(n, 34, device=gpu, generator=torch.Generator(device=gpu).manual_seed(77)) * 3
    a_det = fused.step(obs, deterministic=True)[0]
    act, val, logp = sampled(fused, obs, row_offset=off)
    check_noise(f"row_offset 2^32-100 {precision}", act, a_det, logp, ac64.log_std,
                policy_normals(SEED, COUNTER, off, np.arange(n)))
    lo = sampled(fused, obs[:100], row_offset=off)
    hi = sampled(fused, obs[100:], row_offset=0)
    for got, a, b in zip((act, val, logp), lo, hi):
        assert torch.equal(got, torch.cat([a, b]))


@pytest.mark.gpu
def test_policy_counter_wraps(gpu):
    """The call counter is taken mod 2^32: steps at counter 0xFFFFFFFF and the next draw the noise
    of counters 0xFFFFFFFF and 0."""
    ac, fused, ac64 = network(gpu, 34, "bf16x3")
    obs = torch.randn(2049, 34, device=gpu, generator=torch.Generator(device=gpu).manual_seed(78)) * 3
    a_det = fused.step(obs, deterministic=True)[0]
    fused.counter = 0xFFFFFFFF
    first = fused.step(obs)
    second = fused.step(obs)
    for tag, c, (act, _, logp) in (("counter 0xFFFFFFFF", 0xFFFFFFFF, first), ("counter 2^32 -> 0", 0, second)):
        check_noise(tag, act, a_det, logp, ac64.log_std, policy_normals(SEED, c, 0, np.arange(2049)))
    assert not torch.equal(first[0], second[0])


SENTINEL = -7.25
SMALL_CASES = [(34, "fp32"), (34, "bf16x3"), (42, "bf16x3")]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 127, 128, 129, 2049])
@pytest.mark.parametrize("obs_dim,precision", SMALL_CASES)
def test_policy_small_and_ragged_into_views(gpu, obs_dim, precision, n):
    """step_into on views of larger buffers (one guard row before, two after; the observation guards
    are NaN, the output guards a sentinel): mu, V and noise as at the large size, guards untouched."""
    ac, fused, ac64 = network(gpu, obs_dim, precision)
    g = torch.Generator(device=gpu).manual_seed(10 * n + obs_dim)
    obs_buf = torch.full((n + 3, obs_dim), float("nan"), device=gpu)
    obs_buf[1:n + 1] = torch.randn(n, obs_dim, device=gpu, generator=g) * 3
    obs = obs_buf[1:n + 1]
    act_buf = torch.full((n + 3, 4), SENTINEL, device=gpu)
    val_buf = torch.full((n + 3,), SENTINEL, device=gpu)
    lp_buf = torch.full((n + 3,), SENTINEL, device=gpu)
    act, val, logp = act_buf[1:n + 1], val_buf[1:n + 1], lp_buf[1:n + 1]
    assert act.data_ptr() % 16 == 0 and obs.data_ptr() % 8 == 0 and obs.is_contiguous()
    a_det, v_det, _ = fused.step(obs, deterministic=True)
    fused.counter = COUNTER
    fused.step_into(obs, act, val, logp, row_offset=11)
    for buf in (act_buf, val_buf, lp_buf):
        guards = torch.cat([buf[:1], buf[n + 1:]])
        assert torch.equal(guards, torch.full_like(guards, SENTINEL)), "a guard row was written"
    mu_ref, v_ref = reference64(ac64, obs)
    e_mu, e_v = float(mixed_err(a_det, mu_ref).max()), float(mixed_err(val, v_ref).max())
    print(f"PARITY small D={obs_dim} {precision} n={n}: mu {e_mu:.3e} V {e_v:.3e}")
    assert e_mu < POLICY_TOL[precision] and e_v < POLICY_TOL[precision]
    assert torch.equal(val, v_det)
    check_noise(f"small D={obs_dim} {precision} n={n}", act, a_det, logp, ac64.log_std,
                policy_normals(SEED, COUNTER, 11, np.arange(n)))


# ---------------------------------------------------------------- masked value pass (GPU)
def mask_patterns(geo):
    n = geo["n"]
    block3 = geo["block"] == 3
    last = geo["chunk"] == geo["nchunks"] - 1
    return [("every row", np.ones(n, np.uint8)), ("block 3 only", block3.astype(np.uint8)),
            ("all but block 3", (~block3).astype(np.uint8)), ("ragged last chunk only", last.astype(np.uint8)),
            ("kk = 4 only", (geo["kk"] == 4).astype(np.uint8)), ("nothing", np.zeros(n, np.uint8)),
            ("every row, bytes 2 and 255", np.where(np.arange(n) % 3 == 0, 2, 255).astype(np.uint8))]


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dim,precision", DIMS_PRECS)
def test_value_masked_patterns_over_several_trips(gpu, obs_dim, precision):
    """Mode 1 at the edge row count: unmarked rows keep the sentinel bit for bit, marked rows equal
    mode 0's value bit for bit (the same v-network MFMAs in the same order) and the float64 value
    network within POLICY_TOL -- whichever blocks the per-block scan lets exit early."""
    B = big_case(gpu, obs_dim, precision)
    fused = network(gpu, obs_dim, precision)[1]
    assert B["geo"]["blocks"] > 3
    for name, m in mask_patterns(B["geo"]):
        mask = torch.as_tensor(m, device=gpu)
        assert mask.dtype == torch.uint8
        sel = mask != 0
        out = torch.full((B["n"],), SENTINEL, device=gpu)
        fused.value_masked(B["obs"], mask, out)
        kept = out[~sel]
        assert torch.equal(kept, torch.full_like(kept, SENTINEL)), f"{name}: an unmarked row was written"
        got, want = out[sel], B["v_det"][sel]
        missing = int((got == SENTINEL).sum())
        assert missing == 0, f"{name}: {missing} of {int(sel.sum())} marked rows were not written"
        assert torch.equal(got, want), f"{name}: marked rows differ from mode 0's value"
        if got.numel():
            e = float(mixed_err(got, B["v_ref"][sel]).max())
            print(f"PARITY masked D={obs_dim} {precision} {name}: rows {got.numel()} V {e:.3e}")
            assert e < POLICY_TOL[precision]


# ---------------------------------------------------------------- GAE (GPU)
GAMMA, LAM = float(np.float32(0.99)), float(np.float32(0.95))     # the C ABI takes floats: exact here
REW_DEN = 0.75
KINDS = ("no done", "done at every step", "done at t = 0 and t = T - 1", "consecutive dones", "random")


GAE_TS, GAE_NS = [1, 7, 8, 9, 16, 67], [1, 255, 256, 257, 1000]
# reward scaling: off; on with no sample clipped (|r / 0.75| stays far below 10); on with rewards
# x 6 (r / 0.75 ~ 8 sigma: ~10 % of the samples beyond each clip bound)
GAE_CASES = (("off", 1.0, None), ("on, none clipped", 1.0, REW_DEN), ("on, both sides clip", 6.0, REW_DEN))


def gae_variants(N):
    return range(1 if N >= 5 else len(KINDS))


def gae_inputs(T, N, scale, variant):
    """float32 [T, N] inputs with the edge envs at columns 0..3 (N >= 5) or, for N < 5, the edge
    `variant` at column 0.  trunc is a subset of done; trunc_val is NaN wherever trunc is 0.  With
    scale > 1 every 7th sample is +-9 (beyond the clip at rew_den 0.75), so that both sides clip
    at the smallest shapes too."""
    rng = np.random.default_rng(100_000 * variant + 1000 * T + N)
    rew = (rng.normal(size=(T, N)) * scale).astype(np.float32)
    if scale > 1.0:
        k = (np.arange(T * N).reshape(T, N) + variant) % 7
        rew[k == 0], rew[k == 1] = 9.0, -9.0
    val = rng.normal(size=(T, N)).astype(np.float32)
    done = rng.random((T, N)) < 0.15
    trunc_draw = rng.random((T, N)) < 0.4

    def edge(col, kind):
        if kind == 0:
            done[:, col] = False
        elif kind == 1:
            done[:, col] = True
            trunc_draw[:, col] = np.arange(T) % 2 == 0          # time-outs and terminals alternate
        elif kind == 2:
            done[:, col] = False
            done[0, col] = done[T - 1, col] = True
            trunc_draw[0, col], trunc_draw[T - 1, col] = False, T > 1
        elif kind == 3:
            done[:, col] = False
            done[T // 2:T // 2 + 3, col] = True
            trunc_draw[T // 2:T // 2 + 3, col] = [True, False, True][:len(done[T // 2:T // 2 + 3, col])]
    if N >= 5:
        for k in range(4):
            edge(k, k)
    else:
        edge(0, variant)
    trunc = done & trunc_draw
    trunc_val = np.where(trunc, rng.normal(size=(T, N)), np.nan).astype(np.float32)
    last_val = rng.normal(size=N).astype(np.float32)
    return rew, val, done, trunc, trunc_val, last_val


def gae_case_inputs(T, N):
    """Every (case, rew_den, variant, inputs) of one shape, after the host-side coverage conditions:
    the edge envs are what they claim, time-outs and terminals both occur, no sample clips in the
    "none clipped" case and at least 1 % (and at least one) clip on each side in the clipping case."""
    sets, kinds = [], set()
    for case, scale, den in GAE_CASES:
        hi = lo = total = 0
        for variant in gae_variants(N):
            inp = rew, val, done, trunc, trunc_val, last_val = gae_inputs(T, N, scale, variant)
            assert not (trunc & ~done).any()
            assert np.isnan(trunc_val[~trunc]).all() and np.isfinite(trunc_val[trunc]).all()
            cols = {k: k for k in range(4)} if N >= 5 else {variant: 0}
            mid = slice(T // 2, T // 2 + 3)
            if 0 in cols:
                assert not done[:, cols[0]].any()
            if 1 in cols:
                assert done[:, cols[1]].all()
            if 2 in cols:
                assert done[0, cols[2]] and done[T - 1, cols[2]] and done[:, cols[2]].sum() == min(T, 2)
            if 3 in cols:
                assert done[mid, cols[3]].all() and done[:, cols[3]].sum() == min(3, T - T // 2)
            kinds |= ({"time-out"} if trunc.any() else set()) | ({"terminal"} if (done & ~trunc).any() else set())
            z = rew.astype(np.float64) / REW_DEN
            hi, lo, total = hi + int((z > 10).sum()), lo + int((z < -10).sum()), total + z.size
            sets.append((case, den, variant, inp))
        if scale == 1.0:
            assert hi == 0 and lo == 0
        else:
            assert hi >= max(1, 0.01 * total) and lo >= max(1, 0.01 * total), f"{hi} / {lo} of {total} samples clip"
    assert kinds == {"time-out", "terminal"}, kinds
    return sets


@pytest.mark.parametrize("N", GAE_NS)
@pytest.mark.parametrize("T", GAE_TS)
def test_gae_inputs_cover_the_edges(T, N):
    """The coverage conditions of the GAE inputs hold at every shape (checked without a GPU; the GPU
    test runs the same checks on the inputs it uses)."""
    sets = gae_case_inputs(T, N)
    assert len(sets) == 3 * (1 if N >= 5 else len(KINDS))
    assert all(x[3][0].shape == (T, N) and x[3][0].dtype == np.float32 for x in sets)


def inf_rel(g, r):
    """|g - r|_inf / |r|_inf (inf where r is 0 and g is not)"""
    den = float(r.abs().max())
    num = float((g.double() - r).abs().max())
    return num / den if den > 0 else (0.0 if num == 0 else math.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("N", GAE_NS)
@pytest.mark.parametrize("T", GAE_TS)
def test_gae_kernel_edges_against_float64(gpu, T, N):
    """cf2_gae on every env against gae() in float64, with reward scaling off, on without a clipped
    sample and on with both clip sides active, into views of sentinel-filled storage (one guard
    row before, two after).  T below, at and above the 8-step load block; N around the 256-thread
    block."""
    from cf2sim.rollout import gae, gae_device
    dev = lambda x: torch.as_tensor(x, device=gpu)
    for case, den, variant, inputs in gae_case_inputs(T, N):
        what = f"{case}, {'all edge envs' if N >= 5 else KINDS[variant]}"
        r, v, d, tr, tv, lv = [dev(x) for x in inputs]
        ref = gae(r.double(), v.double(), d, tr, lv.double(), tv.double(), GAMMA, LAM, den, True)
        t32 = gae(r, v, d, tr, lv, tv, GAMMA, LAM, den, True)
        store = torch.full((3, T + 3, N), SENTINEL, device=gpu)
        outs = tuple(store[k, 1:T + 1] for k in range(3))
        d8, tr8 = d.to(torch.uint8), tr.to(torch.uint8)
        got = gae_device(r, v, d8, tr8, lv, tv, GAMMA, LAM, den, True, out=outs)
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
        guards = torch.cat([store[:, :1], store[:, T + 1:]], dim=1)
        assert torch.equal(guards, torch.full_like(guards, SENTINEL)), f"{what}: a guard row was written"
        for name, g, r64, r32 in zip(("adv", "ret", "disc"), got, ref, t32):
            assert torch.isfinite(r64).all()
            assert torch.isfinite(g).all(), f"{name} ({what}) is not finite: trunc_val read where trunc is 0?"
            ek, e32 = inf_rel(g, r64), inf_rel(r32, r64)
            if variant == 0:
                print(f"PARITY gae T={T} N={N} {case} {name}: kernel {ek:.3e} torch-fp32 {e32:.3e}")
            assert ek <= max(8 * e32, FLOOR), f"{name} ({what}): kernel {ek:.3e}, torch fp32 {e32:.3e}"
        # without with_discounted, a disc buffer that was passed in stays untouched
        store2 = torch.full((3, T, N), SENTINEL, device=gpu)
        a2, r2 = gae_device(r, v, d8, tr8, lv, tv, GAMMA, LAM, den, False, out=tuple(store2))
        assert torch.equal(a2, got[0]) and torch.equal(r2, got[1])
        assert torch.equal(store2[2], torch.full_like(store2[2], SENTINEL)), f"{what}: disc written without with_discounted"
