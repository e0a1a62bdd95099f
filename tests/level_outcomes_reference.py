"""NumPy restatement of cf2_level_outcomes (include/cf2sim.h): per-env carries as sequential f32 /
int32 adds in time order, episodes binned by the bits of their level, rows in fp64.

The row sums are exactly rounded (math.fsum), so a tested sum's distance from them is the tested
sum's own rounding error.  ``abs_sums`` holds, per row, the sums of |v| (and of v^2) that the
summation-order bound m * 2^-52 * sum|v| is built from."""
import math

import numpy as np

WORDS = 16


def empty_table(L):
    t = np.zeros((L + 1, WORDS))
    t[:, [3, 7, 11]], t[:, [4, 8, 12]] = np.inf, -np.inf
    return t


def bin_of(level_bits, table_bits):
    """Row of a level: the first table entry with the same bits, else len(table) ("other")."""
    hit = np.nonzero(table_bits == level_bits)[0]
    return int(hit[0]) if hit.size else int(table_bits.size)


def episodes(rew, done, level_values, cost=None, trunc=None, level=None, carry=None, episodes_left=None):
    """Scan [T, n] forward in time.  Returns (list of recorded episodes (bin, ret f32, len int, cost f32,
    crash, timeout, t, env), (carry_ret f32 [n], carry_cost f32 [n], carry_len int32 [n]), episodes_left)."""
    rew = np.asarray(rew, dtype=np.float32)
    T, n = rew.shape
    done = np.asarray(done).astype(np.uint8)
    lv_bits = np.asarray(level_values, dtype=np.float32).view(np.uint32)
    if carry is None:
        carry = (np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32))
    er, ec, el = (np.array(c, copy=True) for c in carry)
    assert er.dtype == np.float32 and ec.dtype == np.float32 and el.dtype == np.int32
    left = None if episodes_left is None else np.array(episodes_left, dtype=np.int32, copy=True)
    out = []
    for t in range(T):
        er = er + rew[t]                                  # f32 + f32 -> f32, one rounding, as the kernel's add
        if cost is not None:
            ec = ec + np.asarray(cost[t], dtype=np.float32)
        el = el + np.int32(1)
        for e in np.nonzero(done[t])[0]:
            if left is None or left[e] > 0:
                b = 0 if level is None else bin_of(np.float32(level[t][e]).view(np.uint32), lv_bits)
                tr = trunc is not None and trunc[t][e] != 0
                out.append((b, er[e], int(el[e]), ec[e], trunc is not None and not tr, tr, t, int(e)))
                if left is not None:
                    left[e] -= 1
            er[e], ec[e], el[e] = 0.0, 0.0, 0
    return out, (er, ec, el), left


def table_of(eps, L):
    """(table [L + 1, 16] f64, abs_sums [L + 1, 6]: sum |v| and sum v^2 of return, length, cost)."""
    table, abs_sums = empty_table(L), np.zeros((L + 1, 6))
    for b in range(L + 1):
        mine = [e for e in eps if e[0] == b]
        if not mine:
            continue
        row = table[b]
        row[0] = len(mine)
        row[13] = sum(1 for e in mine if e[4])
        row[14] = sum(1 for e in mine if e[5])
        for j, col in enumerate((1, 2, 3)):
            v = [float(e[col]) for e in mine]              # f32 / int -> f64: exact
            row[1 + 4 * j] = math.fsum(v)
            row[2 + 4 * j] = math.fsum(x * x for x in v)   # x * x is exact in f64 for f32 and int32 lengths
            row[3 + 4 * j], row[4 + 4 * j] = min(v), max(v)
            abs_sums[b, 2 * j] = math.fsum(abs(x) for x in v)
            abs_sums[b, 2 * j + 1] = row[2 + 4 * j]
    return table, abs_sums


def merge_tables(a, b):
    """b merged into a copy of a, per row (accumulate != 0): counts and sums add, min / max combine."""
    out = np.array(a, copy=True)
    for k in range(out.shape[0]):
        if not b[k, 0] > 0:
            continue
        if not out[k, 0] > 0:
            out[k] = b[k]
            continue
        for j in (0, 13, 14, 1, 2, 5, 6, 9, 10):
            out[k, j] += b[k, j]
        for j in (3, 7, 11):
            out[k, j] = min(out[k, j], b[k, j])
            out[k, j + 1] = max(out[k, j + 1], b[k, j + 1])
    return out


def level_outcomes(rew, done, level_values, **kw):
    """One call of cf2_level_outcomes on fresh or given carries: (table, abs_sums, carries, episodes_left, eps)."""
    eps, carry, left = episodes(rew, done, level_values, **kw)
    table, abs_sums = table_of(eps, len(np.asarray(level_values).reshape(-1)))
    return table, abs_sums, carry, left, eps


SUM_WORDS = ((1, 0), (2, 1), (5, 2), (6, 3), (9, 4), (10, 5))     # (table word, abs_sums column)
EXACT_WORDS = (0, 3, 4, 7, 8, 11, 12, 13, 14, 15)


def check_table(got, ref, abs_sums):
    """Counts, crashes, time-outs, min and max equal; every sum within m * 2^-52 * sum|v| (m the row's
    count): the bound on the difference of two fp64 summation orders of the same m terms, (m - 1) u
    sum|v| each with u = 2^-53, nothing looser.  Raises AssertionError naming the row and word."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for k in range(ref.shape[0]):
        for w in EXACT_WORDS:
            assert got[k, w] == ref[k, w], f"row {k} word {w}: {got[k, w]!r} != {ref[k, w]!r}"
        for w, c in SUM_WORDS:
            bound = ref[k, 0] * 2.0 ** -52 * abs_sums[k, c]
            assert abs(got[k, w] - ref[k, w]) <= bound, \
                f"row {k} word {w}: |{got[k, w]!r} - {ref[k, w]!r}| > {bound!r}"
