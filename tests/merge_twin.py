"""Numpy restatement of the az_samples_merge contract (include/az_engine.h): position averaging.  Nothing here is
shared with the engine.  TEST INFRASTRUCTURE ONLY.

  key      Game::pack(s) = mine + (mine | theirs) + bottom row; canonical: of c(s), the mirror rule of tests/mirror_twin.py
  order    groups in order of first occurrence
  k = 1    the tuple verbatim (canonicalised under `canonical`: pi reversed when the state is the mirrored one)
  k > 1    S = sum of rint(x * 2^38) in int64 per value; mean = float32(float64(S) / float64(k * 2^38)), no renormalisation"""
import numpy as np

import mirror_twin as mt

FRAC = 2.0 ** 38
MAX_TUPLES = 1 << 24
BOARD_MASK = np.uint64(sum(0x3F << (7 * c) for c in range(7)))
DRAW_EPS = np.float32(1e-4)


def quantise(x):
    """q(x) = llrint((double)x * 2^38): the product is exact, rint rounds to nearest even."""
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * FRAC).astype(np.int64)


def mean_of(sums, k):
    """(float)((double)S / (double)(k * 2^38)); k may be an array broadcast against sums."""
    div = (np.asarray(k, np.int64) << np.int64(38)).astype(np.float64)
    return (np.asarray(sums, np.int64).astype(np.float64) / div).astype(np.float32)


def refusal(pis, zs, *, states=None, boards=None, capacity=None, flags=0):
    """The refusal predicates on the data and the scalar arguments: None when the call is legal, else the reason."""
    n = len(zs)
    if flags & ~1:
        return "unknown flag bits"
    if n > MAX_TUPLES:
        return "n > 2^24"
    if capacity is not None and capacity < n:
        return "capacity < n"
    for x in (np.asarray(pis, np.float32), np.asarray(zs, np.float32)):
        if np.isnan(x).any():
            return "NaN"
        if ((x < -1) | (x > 1)).any():
            return "value outside [-1, 1]"
    if states is None:
        b = np.asarray(boards, np.float32).reshape(-1, 2, 6, 7)
        if not ((b == 0) | (b == 1)).all():
            return "feature not 0 or 1"
        if ((b[:, 0] == 1) & (b[:, 1] == 1)).any():
            return "both planes set"
        states = mt.boards_to_states(b)
    s = np.asarray(states, np.uint64).reshape(-1, 2)
    if (s[:, 0] & s[:, 1]).any():
        return "overlapping stones"
    if ((s[:, 0] | s[:, 1]) & ~BOARD_MASK).any():
        return "bits outside the board"
    return None


def merge(pis, zs, *, states=None, boards=None, canonical=False):
    """dict(count, states [m,2] u64, boards [m,2,6,7] f32, pis [m,7] f32, zs [m] f32, counts [m] u32) of a legal input."""
    pis = np.ascontiguousarray(pis, np.float32).reshape(-1, 7)
    zs = np.ascontiguousarray(zs, np.float32).reshape(-1)
    if states is None:
        states = mt.boards_to_states(boards)
    s = np.ascontiguousarray(states, np.uint64).reshape(-1, 2)
    n = len(zs)
    assert refusal(pis, zs, states=s) is None and len(s) == n == len(pis)
    if canonical:
        s, flags = mt.canonical_batch(s)
        m = flags.astype(bool)
        pis = pis.copy()
        pis[m] = pis[m][:, ::-1]
    if n == 0:
        return {"count": 0, "states": s, "boards": mt.states_to_boards(s), "pis": pis, "zs": zs, "counts": np.zeros(0, np.uint32)}
    keys = mt.pack_batch(s)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")              # unique's groups, reordered by first occurrence
    rank_of = np.empty_like(order)
    rank_of[order] = np.arange(len(order))
    group = rank_of[inverse.reshape(-1)]
    first = first[order]
    m = len(first)
    counts = np.bincount(group, minlength=m).astype(np.int64)
    sums = np.zeros((m, 8), np.int64)
    np.add.at(sums, group, quantise(np.concatenate([pis, zs[:, None]], axis=1)))
    mean = mean_of(sums, counts[:, None])
    single = counts == 1
    out_p, out_z = mean[:, :7].copy(), mean[:, 7].copy()
    out_p[single], out_z[single] = pis[first[single]], zs[first[single]]          # verbatim rows
    out_s = s[first]
    return {"count": m, "states": out_s, "boards": mt.states_to_boards(out_s), "pis": out_p, "zs": out_z, "counts": counts.astype(np.uint32)}


def random_positions(rng, n, max_plies=30):
    """n DISTINCT legal positions (stones stacked from the bottom; the side to move is `mine`), [n, 2] uint64."""
    seen, out = set(), []
    while len(out) < n:
        mine = theirs = 0
        for _ in range(int(rng.integers(0, max_plies + 1))):
            mask = mine | theirs
            cols = [c for c in range(7) if not (mask >> (c * 7 + 5)) & 1]
            a = int(rng.choice(cols))
            nb = (mask + (1 << (a * 7))) & (0x3F << (a * 7))
            mine, theirs = theirs, mine | nb
        if (mine, theirs) not in seen:
            seen.add((mine, theirs))
            out.append((mine, theirs))
    return np.array(out, np.uint64).reshape(-1, 2)


def random_targets(rng, n):
    """pi rows (f32, positive, sum about 1) and z from {+1, -1, DRAW_EPS, -DRAW_EPS}."""
    p = rng.random((n, 7)).astype(np.float32) + np.float32(1e-3)
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    z = rng.choice(np.array([1, -1, DRAW_EPS, -DRAW_EPS], np.float32), n).astype(np.float32)
    return p, z
