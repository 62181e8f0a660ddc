"""Dirichlet root noise without a GPU: the twin (tests/cpp/selfplay_twin.cpp: the oracle's search with the noise restated around it) against
the unchanged oracle, the sampler of csrc/az_noise.h (its g++ build) against the Dirichlet distribution, its polynomials against
float64, the mixing formula, and the hosts' plumbing."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import selfplay_twin as tw      # noqa: E402

SALT = 4242


def _full_columns(k):
    """A position whose first k columns are full (only its valid-move mask and stone count matter to the sampler)."""
    mine = theirs = 0
    for c in range(k):
        for r in range(6):
            if (r + c) & 1:
                mine |= 1 << (c * 7 + r)
            else:
                theirs |= 1 << (c * 7 + r)
    return mine, theirs


# ---- 1. the twin is the oracle when the noise is off ------------------------------------------------------------------------------------
@pytest.mark.parametrize("game_kind", [tw.GAME_BITS, tw.GAME_CONNECT3], ids=["connect4", "connect3"])
def test_twin_episodes_equal_the_oracle_at_eps_0(oracle, game_kind):
    n, sims = 32, 25
    for sim_threads in (1, 5):
        ref = oracle.selfplay(n, sims, net_kind=oracle.NET_HASH, salt=SALT, seed=7, first_game_id=3, game_kind=game_kind, sim_threads=sim_threads)
        got = tw.selfplay(n, sims, net_kind=tw.NET_HASH, salt=SALT, seed=7, first_game_id=3, game_kind=game_kind, sim_threads=sim_threads, eps=0.0, alpha=0.3)
        assert got["count"] == ref["count"]
        for k in ("game_len", "moves", "boards", "pis", "zs"):
            assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("game_kind", [tw.GAME_BITS, tw.GAME_CONNECT3], ids=["connect4", "connect3"])
@pytest.mark.parametrize("threads", [1, 4])
def test_twin_search_equals_the_oracle_at_eps_0(oracle, game_kind, threads):
    sims = 40
    ended = oracle.c3_ended if game_kind == tw.GAME_CONNECT3 else oracle.c4_ended
    rng = np.random.default_rng(1)
    for g in range(8):
        a = oracle.Tree(sims, net_kind=oracle.NET_HASH, salt=SALT, game_kind=game_kind, threads=threads)
        b = tw.Tree(sims, net_kind=tw.NET_HASH, salt=SALT, game_kind=game_kind, threads=threads)
        s = (0, 0)
        for move in range(42):
            temp = 1.0 if move < 6 else 0.0
            ra = a.get_action_prob(s[0], s[1], temp, seed=5, game_id=g)
            rb = b.get_action_prob(s[0], s[1], temp, seed=5, game_id=g, eps=0.0)
            for x, y in zip(ra, rb):
                assert np.array_equal(x, y), (g, move)
            s = oracle.c4_play(s[0], s[1], int(rng.choice([i for i in range(7) if ra[0][i] > 0])))
            if ended(*s) != 0.0:
                break


# ---- 2. the sampler is a Dirichlet sampler ------------------------------------------------------------------------------------------------
def _ks_two_sample(x, y):
    x, y = np.sort(x), np.sort(y)
    grid = np.concatenate([x, y])
    return float(np.max(np.abs(np.searchsorted(x, grid, side="right") / len(x) - np.searchsorted(y, grid, side="right") / len(y))))


@pytest.mark.parametrize("alpha", [0.3, 1.0, 1.4, 10.0])
@pytest.mark.parametrize("full_cols", [0, 3], ids=["7-moves", "4-moves"])
def test_sampler_statistics(alpha, full_cols):
    N = 200_000
    k = 7 - full_cols
    s = _full_columns(full_cols)
    eta = tw.noise_eta(np.tile(np.array(s, np.uint64), (N, 1)), np.arange(N, dtype=np.uint64), alpha, seed=11)
    assert np.isfinite(eta).all() and (eta >= 0).all()
    assert (eta[:, :full_cols] == 0).all() and (eta[:, full_cols:] > 0).any()
    assert np.max(np.abs(eta.astype(np.float64).sum(axis=1) - 1.0)) <= 1e-6
    var = (k - 1) / (k * k * (k * alpha + 1))
    z = np.abs(eta[:, full_cols:].astype(np.float64).mean(axis=0) - 1.0 / k) / math.sqrt(var / N)
    ref = np.random.default_rng(2024).dirichlet([alpha] * k, N)[:, 0]
    D = _ks_two_sample(eta[:, full_cols].astype(np.float64), ref)
    print(f"alpha {alpha} k {k}: max z {z.max():.2f}  KS D {D:.4f} (bound {2.69 * math.sqrt(2 / N):.4f})")
    assert z.max() <= 6.0, z
    assert D <= 2.69 * math.sqrt(2.0 / N), D


def test_sampler_is_a_function_of_its_stream_alone():
    """eta depends on (seed, game id, ply, alpha, mask): the same roots in another order give the same rows, another seed or other
    game ids give other rows."""
    ids = np.arange(64, dtype=np.uint64)
    st = np.tile(np.array(_full_columns(2), np.uint64), (64, 1))
    a = tw.noise_eta(st, ids, 0.3, seed=3)
    b = tw.noise_eta(st[::-1], ids[::-1], 0.3, seed=3)
    assert np.array_equal(a, b[::-1])
    assert not np.array_equal(a, tw.noise_eta(st, ids, 0.3, seed=4))
    assert not np.array_equal(a, tw.noise_eta(st, ids + 64, 0.3, seed=3))


# ---- 3. the polynomials ---------------------------------------------------------------------------------------------------------------------
def test_log2_and_exp2_accuracy():
    """Over the ranges the sampler uses: log2 of s = v1^2 + v2^2 >= 2^-47, of v^3 down to the smallest normal, of the uniforms
    (>= 2^-25), exp2 of log2(u) / alpha in [-125, 0].  Relative error <= 1e-5 is the sampler's need (it perturbs an acceptance
    probability far below what the statistics above resolve); the measured maxima are in the header of csrc/az_noise.h."""
    rng = np.random.default_rng(0)
    x = np.concatenate([np.exp2(rng.uniform(-126, 24, 400_000)), 1.0 + rng.uniform(-1e-3, 1e-3, 100_000), np.exp2(rng.uniform(-1, 1, 200_000)),
                        np.nextafter(np.float32(1), np.float32([0, 2])), np.exp2(np.arange(-126, 25, dtype=np.float64))]).astype(np.float32)
    x = x[x != 1.0]
    got = tw.noise_log2(x).astype(np.float64)
    ref = np.log2(x.astype(np.float64))
    e_log = float(np.max(np.abs(got - ref) / np.abs(ref)))
    assert tw.noise_log2(np.float32([1.0]))[0] == 0.0
    y = np.concatenate([rng.uniform(-124.999, 0, 400_000), -np.exp2(rng.uniform(-30, 0, 100_000)), np.arange(-124, 1, dtype=np.float64)]).astype(np.float32)
    got = tw.noise_exp2(y).astype(np.float64)
    ref = np.exp2(y.astype(np.float64))
    e_exp = float(np.max(np.abs(got - ref) / ref))
    print(f"max relative error: log2 {e_log:.3g}, exp2 {e_exp:.3g}")
    assert e_log <= 1e-5 and e_exp <= 1e-5
    assert (tw.noise_exp2(np.float32([-125.0, -126.0, -1e30, -np.inf])) == 0).all() and tw.noise_exp2(np.float32([0.0]))[0] == 1.0


# ---- 4. the mixing formula ------------------------------------------------------------------------------------------------------------------
def test_eps_1_stores_eta_itself(oracle):
    """(1 - 1) * p + 1 * eta[a] = eta[a] bit for bit: the twin's stored root priors are the sampler's output, at the first root (its own
    evaluation arrives in this call) and at a root the tree already knew (expanded, with its prior, by the earlier search)."""
    t = tw.Tree(50, net_kind=tw.NET_HASH, salt=SALT)
    s = (0, 0)
    for move in range(12):
        pi, _, _ = t.get_action_prob(s[0], s[1], 1.0, seed=9, game_id=17, eps=1.0, alpha=0.3)
        eta = tw.noise_eta(np.array([s], np.uint64), [17], 0.3, seed=9)[0]
        assert np.array_equal(t.root_priors(*s).view(np.uint32), eta.view(np.uint32)), move
        s = oracle.c4_play(s[0], s[1], int(np.argmax(pi)))
        if oracle.c4_ended(*s) != 0.0:
            break


def test_eps_quarter_changes_games_and_mixes_as_stated(oracle):
    base = tw.selfplay(32, 25, net_kind=tw.NET_HASH, salt=SALT, seed=7, eps=0.0)
    noisy = tw.selfplay(32, 25, net_kind=tw.NET_HASH, salt=SALT, seed=7, eps=0.25, alpha=0.3)
    differ = [g for g in range(32) if base["game_len"][g] != noisy["game_len"][g] or not np.array_equal(base["moves"][g], noisy["moves"][g])]
    assert differ, "root noise at eps = 0.25 changed none of 32 games"
    again = tw.selfplay(32, 25, net_kind=tw.NET_HASH, salt=SALT, seed=7, eps=0.25, alpha=0.3)
    assert np.array_equal(noisy["moves"], again["moves"]) and np.array_equal(noisy["pis"], again["pis"])
    # the stored prior of a fresh root is fadd(fmul(fsub(1, eps), p), fmul(eps, eta)) of the masked, renormalised net prior
    t = tw.Tree(10, net_kind=tw.NET_HASH, salt=SALT)
    t.get_action_prob(0, 0, 1.0, seed=1, game_id=2, eps=0.25, alpha=1.4)
    p, _ = oracle.hashnet(0, 0, SALT)
    ssum = np.float32(0)
    for a in range(7):
        ssum = np.float32(ssum + p[a])
    p = (p / ssum).astype(np.float32)
    eta = tw.noise_eta(np.array([[0, 0]], np.uint64), [2], 1.4, seed=1)[0]
    eps = np.float32(tw.e6(0.25) / 1e6)
    want = ((np.float32(1) - eps) * p).astype(np.float32) + (eps * eta).astype(np.float32)
    assert np.array_equal(t.root_priors(0, 0).view(np.uint32), want.astype(np.float32).view(np.uint32))


# ---- 5. the hosts forward the parameters ----------------------------------------------------------------------------------------------------
def test_python_coach_forwards_root_noise():
    """coach.Coach sets the two options around self-play only: on before the episodes, off before the gate."""
    import alphazero_rs_amd.coach as coach_mod

    calls = []

    class FakeEngine:
        def set_root_noise(self, eps, alpha=1.0):
            calls.append(("noise", eps, alpha))

    c = coach_mod.Coach.__new__(coach_mod.Coach)
    c.engine = FakeEngine()
    c.root_noise_eps, c.root_noise_alpha = 0.25, 0.3
    with c._selfplay_root_noise():
        calls.append(("selfplay",))
    assert calls == [("noise", 0.25, 0.3), ("selfplay",), ("noise", 0.0, 0.3)]
    c.root_noise_eps = 0.0
    calls.clear()
    with c._selfplay_root_noise():
        calls.append(("selfplay",))
    assert calls == [("selfplay",)]          # off: the engine is never asked (hosts written before the option keep working)


def test_cpp_coach_forwards_root_noise(tmp_path):
    exe = str(tmp_path / "test_root_noise_host_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_root_noise_host_cpu.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe, str(tmp_path / "coach")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
