"""Gumbel root search with sequential halving ("gumbel_m", include/az_engine.h) without a GPU: csrc/az_gumbel.h -- the text the tree kernels
compile -- as g++ builds it (tests/cpp/gumbel_twin.cpp), held to independent restatements: the considered-visit sequence to the list
construction of the published implementation, the variates to float64, every formula to numpy f32 element by element; and the twin's
episodes at the shapes the GPU tests use: every simulation finds a considered slot, the visits of a move are the prescribed schedule, and
every counter the GPU parity tests lean on is non-zero."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gumbel_twin as gt        # noqa: E402

f32 = np.float32
HASH_SALT, MODEL_SALT = 1234, 0x51ED27
# (m, sims, seed) of tests/test_gumbel_gpu.py
SHAPES = ((2, 8, 11), (4, 16, 12), (7, 33, 13))


# ---- the considered-visit sequence ------------------------------------------------------------------------------------------------------------
def sequence_of_considered_visits(m, n):
    """The list construction of sequential halving's schedule (mctx, seq_halving.get_sequence_of_considered_visits), restated."""
    if m <= 1:
        return list(range(n))
    log2max = int(math.ceil(math.log2(m)))
    seq, visits, k = [], [0] * m, m
    while len(seq) < n:
        extra = max(1, int(n / (log2max * k)))
        for _ in range(extra):
            seq.extend(visits[:k])
            for i in range(k):
                visits[i] += 1
        k = max(2, k // 2)
    return seq[:n]


def test_considered_visit_is_the_published_sequence():
    for m in range(1, 8):
        for n in range(1, 401):
            assert gt.considered(m, n).tolist() == sequence_of_considered_visits(m, n), (m, n)


def prescribed_py(m_eff, n, nchild):
    """How often each of the nchild slots is visited, largest first: slot i of a phase with k considered actions is visited when the
    sequence asks for the i-th of them."""
    if m_eff <= 1:
        return [n] + [0] * (nchild - 1)
    log2max = int(math.ceil(math.log2(m_eff)))
    d, k, left = [0] * nchild, m_eff, n
    while left > 0:
        extra = max(1, int(n / (log2max * k)))
        for _ in range(extra):
            for i in range(k):
                if left > 0:
                    d[i] += 1
                    left -= 1
        k = max(2, k // 2)
    return d


def test_prescribed_visits_of_the_twin():
    for nchild in range(1, 8):
        for m in range(2, 8):
            for n in (1, 2, 7, 8, 16, 33, 100):
                m_eff = min(m, nchild)
                want = prescribed_py(m_eff, n, nchild)
                assert gt.prescribed_d(m_eff, n, nchild).tolist() == want and sum(want) == n, (nchild, m, n)
                assert want == sorted(want, reverse=True)


# ---- numpy f32 restatement of the header (every operation rounds once to f32) ---------------------------------------------------------------------
def log2_py(x):
    u = int(np.asarray(x, f32).view(np.uint32))
    e = (u >> 23) - 127
    mb = (u & 0x007FFFFF) | 0x3F800000
    if mb >= 0x3FB504F3:
        mb -= 0x00800000
        e += 1
    m = np.asarray(mb, np.uint32).view(f32)
    s = f32(f32(m - f32(1)) / f32(m + f32(1)))
    z = f32(s * s)
    p = f32(0.111111111)
    for c in (0.142857143, 0.2, 0.333333333, 1.0):
        p = f32(f32(p * z) + f32(c))
    ln_m = f32(f32(f32(2) * s) * p)
    return f32(f32(e) + f32(ln_m * f32(1.44269504)))


def ln_py(x):
    return f32(log2_py(x) * f32(0.693147182))


def exp2_py(x):
    x = f32(x)
    if not x > f32(-125):
        return f32(0)
    if x > 0:
        x = f32(0)
    n = int(f32(x - f32(0.5)))          # truncation toward zero, as the C cast
    t = f32(f32(x - f32(n)) * f32(0.693147182))
    p = f32(1.98412698e-4)
    for c in (1.38888889e-3, 8.33333333e-3, 4.16666667e-2, 0.166666667, 0.5, 1.0, 1.0):
        p = f32(f32(p * t) + f32(c))
    return np.asarray((int(p.view(np.uint32)) + ((n << 23) & 0xFFFFFFFF)) & 0xFFFFFFFF, np.uint32).view(f32)


def uniform_py(r):
    return f32(f32(f32(r >> 41) + f32(0.5)) * f32(2.0 ** -23))


def of_uniform_py(u):
    return f32(-ln_py(f32(-ln_py(u))))


def logit_py(p):
    tiny = f32(1.17549435e-38)
    return ln_py(p if p > tiny else tiny)


def sigmas_py(p, q, n, c_visit, c_scale):
    num = den = f32(0)
    for pj, qj, nj in zip(p, q, n):
        if nj > 0:
            num = f32(num + f32(pj * qj))
            den = f32(den + pj)
    v_mix = f32(num / den) if den > 0 else f32(0)
    scale = f32(f32(f32(c_visit) + f32(max(n))) * f32(c_scale))
    return [f32(scale * (qj if nj > 0 else v_mix)) for qj, nj in zip(q, n)]


def argmax_py(p, g, sigma, d, want):
    best, bu, found = 0, None, False
    for j in range(len(p)):
        ok = d[j] == want
        u = f32(f32(g[j] + logit_py(p[j])) + sigma[j]) if ok else f32(-np.inf)
        found = found or ok
        if j == 0 or not bu > u:
            best, bu = j, u
    return best, found


def root_py(p, q, g, n, base, m, budget, c_visit, c_scale):
    d = [(int(a) - int(b)) & 0xFFFF for a, b in zip(n, base)]
    sigma = sigmas_py(p, q, n, c_visit, c_scale)
    m_eff = min(m, len(p))
    t = sum(d)
    sel, found = argmax_py(p, g, sigma, d, sequence_of_considered_visits(m_eff, budget)[t]) if t < budget else (None, None)
    x = [f32(logit_py(pj) + sj) for pj, sj in zip(p, sigma)]
    mx = max(x)
    e = [exp2_py(f32(f32(xj - mx) * f32(1.44269504))) for xj in x]
    tot = f32(0)
    for ej in e:
        tot = f32(tot + ej)
    pi = [f32(ej / tot) for ej in e]
    res, _ = argmax_py(p, g, sigma, d, max(d))
    return sel, found, res, sigma, pi


def test_uniform_is_exact_and_strictly_inside_the_unit_interval():
    r = np.array([0, (1 << 64) - 1, 1 << 41, (1 << 63), 0x123456789ABCDEF0], np.uint64)
    u = gt.uniform(r)
    for ri, ui in zip(r.tolist(), u.tolist()):
        assert ui == ((ri >> 41) + 0.5) * 2.0 ** -23          # exact: the f32 equals the rational
        assert 0.0 < ui < 1.0
        assert uniform_py(ri) == f32(ui)
    assert u[0] == 2.0 ** -24 and u[1] == 1.0 - 2.0 ** -24


# csrc/az_gumbel.h states it: the inner logarithm's relative error e (2.7e-7 of noise_log2 plus the rounding of the ln 2 product, 6e-8)
# becomes an absolute e in the outer logarithm, which adds e * |g| of its own: e * (1 + |g|) <= 2 * 3.3e-7 * max(1, |g|)
G_BOUND = 6.6e-7


def test_variate_against_float64():
    rng = np.random.default_rng(5)
    k = np.concatenate([np.arange(0, 4096), np.arange((1 << 23) - 4096, 1 << 23), rng.integers(0, 1 << 23, 1 << 20),
                        int(math.exp(-1.0) * 2 ** 23) + np.arange(-4096, 4096)]).astype(np.uint64)
    u = gt.uniform(k << np.uint64(41))
    g = gt.of_uniform(u).astype(np.float64)
    exact = -np.log(-np.log(u.astype(np.float64)))
    err = np.abs(g - exact) / np.maximum(1.0, np.abs(exact))
    print("largest |g - exact| / max(1, |exact|): %.3g at U = %.9g; g in [%.4f, %.4f]" % (err.max(), u[err.argmax()], g.min(), g.max()))
    assert np.isfinite(g).all()
    assert err.max() <= G_BOUND
    for ui in u[:8].tolist() + u[-8:].tolist():
        assert of_uniform_py(f32(ui)) == gt.of_uniform(np.array([ui], f32))[0]


def test_numpy_restatement_equals_the_host_build():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.random(2000).astype(f32), f32(2.0) ** rng.integers(-126, 2, 200).astype(f32), [f32(1.17549435e-38), f32(1.0), f32(0.0)]]).astype(f32)
    got = gt.logit(x)
    for xi, gi in zip(x, got):
        assert logit_py(f32(xi)).view(np.uint32) == gi.view(np.uint32), xi
    for trial in range(400):
        nchild = int(rng.integers(1, 8))
        m, budget = int(rng.integers(2, 8)), int(rng.choice([8, 16, 33, 100]))
        p = rng.dirichlet(np.ones(nchild) * 0.5).astype(f32)
        if trial % 7 == 0:
            p[int(rng.integers(0, nchild))] = 0.0
        base = rng.integers(0, 40, nchild).astype(np.uint32)
        # a state the schedule can reach: the first t entries of the sequence spread over slots in some order
        m_eff = min(m, nchild)
        t = int(rng.integers(0, budget + 1))
        d = np.zeros(nchild, np.uint32)
        order = rng.permutation(nchild)
        for c in sequence_of_considered_visits(m_eff, budget)[:t]:
            j = next(int(o) for o in order if d[o] == c)
            d[j] += 1
        n = base + d
        q = np.where(n > 0, rng.uniform(-1, 1, nchild), 0.0).astype(f32)
        g = gt.of_uniform(gt.uniform(rng.integers(0, 1 << 63, nchild).astype(np.uint64) << np.uint64(1))) if trial % 3 else np.zeros(nchild, f32)
        cv, cs = float(rng.choice([50.0, 0.0, 12.5])), float(rng.choice([1.0, 0.1, 3.0]))
        sel, found, res, sigma, pi = gt.root(p, q, g, n, base, m, budget, cv, cs)
        psel, pfound, pres, psigma, ppi = root_py(list(p), list(q), list(g), n.tolist(), base.tolist(), m, budget, cv, cs)
        if t < budget:
            assert (sel, found) == (psel, pfound) and found, trial
        assert res == pres, trial
        assert np.array_equal(np.array(psigma, f32).view(np.uint32), sigma.view(np.uint32)), trial
        assert np.array_equal(np.array(ppi, f32).view(np.uint32), pi.view(np.uint32)), trial
        assert abs(float(pi.astype(np.float64).sum()) - 1.0) <= 4 * 2.0 ** -23


# ---- the twin's searches ------------------------------------------------------------------------------------------------------------------------
def c4_play(mine, theirs, a):
    mask = mine | theirs
    nb = (mask + (1 << (a * 7))) & (0x3F << (a * 7))
    return theirs, mine | nb


@pytest.mark.parametrize("temp", [1.0, 0.0])
def test_tree_calls_follow_the_schedule(temp):
    """Two calls on the same root (the second one's baseline is non-zero), then a move later: the visits of each call are the prescribed
    ones, the selected action has the most of them, pi sums to 1 and is 0 on invalid actions, counts stay raw."""
    for m, sims, seed in SHAPES:
        tr = gt.Tree(sims, net_kind=gt.NET_HASH, salt=HASH_SALT)
        s = (0, 0)
        # fill column 3 so that it is invalid later
        for a in (3, 3, 3, 3, 3, 3):
            s = c4_play(s[0], s[1], a)
        total = np.zeros(7, np.int64)
        for call in range(3):
            pi, counts, q, sel, d = tr.get_action_prob(s[0], s[1], temp, seed, 40, m=m)
            assert pi[3] == 0.0 and counts[3] == 0 and sel != 3
            assert abs(float(pi.astype(np.float64).sum()) - 1.0) <= 4 * 2.0 ** -23
            assert sorted(d[:6].tolist(), reverse=True) == prescribed_py(min(m, 6), sims, 6) and d[6] == 0
            slots = [a for a in range(7) if a != 3]
            assert d[slots.index(sel)] == d.max()
            if call < 2:
                total += counts
                if call == 1:
                    assert counts.sum() == 2 * sims           # raw: the visits of both calls
            if call == 1:
                s = c4_play(s[0], s[1], sel)
        ctr = gt.counters(tr.ctr)
        assert ctr["no_considered"] == 0 and ctr["bad_schedule"] == 0 and ctr["moves"] == 3 and ctr["moves_reused"] >= 2, ctr
        assert ctr["moves_g_zero"] == (3 if temp == 0.0 else 0)
        tr.close()


@pytest.mark.parametrize("net", ["stub", "hash"])
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_episodes_at_the_gpu_shapes(shape, net):
    """100 episodes per shape: every root selection found a considered slot, every move's visits are the schedule's, and the conditions
    the GPU parity tests assert on hold."""
    m, sims, seed = shape
    kind, salt = (gt.NET_STUB, 0) if net == "stub" else (gt.NET_HASH, HASH_SALT + 10 * MODEL_SALT)
    ref = gt.selfplay(100, sims, m, net_kind=kind, salt=salt, seed=seed, first_game_id=1000)
    c = ref["ctr"]
    print(c)
    assert c["no_considered"] == 0 and c["bad_schedule"] == 0
    assert c["moves"] == int(ref["game_len"].sum()) and c["root_sel"] == sims * c["moves"] == ref["sims"] == ref["budgets"]
    for key in ("root_not_puct", "moves_not_most_visited", "moves_reused", "moves_g_zero"):
        assert c[key] > 0, key
    if net == "hash" and m == 4:         # the baseline repair of a placeholder that becomes a link is rare: this shape meets it 26 times
        assert c["moves_relinked"] >= 10, c
    assert c["moves_g_zero"] < c["moves"]
    pis = ref["pis"].astype(np.float64)
    assert np.abs(pis.sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -23
    full_col = ref["boards"].reshape(-1, 2, 6, 7).sum(axis=(1, 2)) == 6                                 # a full column is an invalid action
    assert (ref["pis"][full_col] == 0).all()        # (short games may have none: test_tree_calls_follow_the_schedule fills a column itself)


def test_combined_with_noise_and_playout_cap():
    ref = gt.selfplay(100, 16, 4, net_kind=gt.NET_HASH, salt=HASH_SALT + 10 * MODEL_SALT, seed=12, first_game_id=1000, eps=0.25, alpha=0.3,
                      cap_sims=5, full_e6=500000)
    c = ref["ctr"]
    full = sum(bin(int(x)).count("1") for x in ref["full_masks"])
    plies = int(ref["game_len"].sum())
    assert 0.1 <= full / plies <= 0.9
    assert c["moves"] == full and c["root_sel"] == 16 * full and ref["budgets"] == 16 * full + 5 * (plies - full) == ref["sims"]
    assert c["no_considered"] == 0 and c["bad_schedule"] == 0 and c["moves_reused"] > 0 and c["root_not_puct"] > 0
