"""Forced playouts and policy target pruning without a GPU ("forced_playouts_k_e6" / "policy_prune", include/az_engine.h): the predicates
of csrc/az_forced.h in their g++ build against a Python restatement in numpy f32, the twin (tests/cpp/selfplay_twin.cpp) against the unchanged
oracle where the two must agree (k = 0), the conditions that keep the GPU parity tests from passing vacuously -- on the seeds and shapes
those tests use --, and the keys and Coach fields on both hosts."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import selfplay_twin as ft      # noqa: E402

HASH_SALT, MODEL_SALT = 1234, 0x51ED27
KEYS = ("forced_playouts_k_e6", "policy_prune")
# the shapes of tests/test_forced_playouts_gpu.py: name -> twin arguments (100 episodes, hash net of model 10, first_game_id 1000)
GPU_SALT = HASH_SALT + 10 * MODEL_SALT
GPU_SHAPES = {
    "fused-24": dict(sims=24, seed=11),
    "graph-44": dict(sims=44, seed=12),
    "dedup-2-24": dict(sims=24, seed=12),
    "four-threads-24": dict(sims=24, seed=11, sim_threads=4),
    "four-threads-per-simulation-24": dict(sims=24, seed=12, sim_threads=4),
    "async-24": dict(sims=24, seed=12),
    "connect-three-25": dict(sims=25, seed=12, game_kind=ft.GAME_CONNECT3),
    "composition": dict(sims=24, seed=11, cap_sims=8, full_e6=500000, eps=0.25, alpha=0.3),
    "composition-four-threads": dict(sims=24, seed=11, cap_sims=8, full_e6=500000, eps=0.25, alpha=0.3, sim_threads=4),
}


def check_conditions(ctr, prune, inflight=False):
    """The issue's conditions on the twin's counters (conditions, not measurements); printed before they are asserted."""
    print({k: ctr[k] for k in ft.COUNTERS})
    assert ctr["root_sel"] > 0 and ctr["root_forced"] >= 0.05 * ctr["root_sel"], ctr
    if inflight:
        assert ctr["root_forced_inflight"] >= 1, ctr
    if prune:
        assert ctr["moves"] > 0 and ctr["moves_pruned"] >= 0.5 * ctr["moves"], ctr
        assert ctr["to_zero"] >= 1, ctr
    else:
        assert ctr["moves_pruned"] == 0 and ctr["visits_pruned"] == 0, ctr


# ---- 1. the predicates ---------------------------------------------------------------------------------------------------------------------
def _cases(n=20000):
    rng = np.random.default_rng(7)
    k_e6 = rng.choice([0, 1, 500000, 2000000, 2000000, 2000000, 16000000, 1234567], n).astype(np.int64)
    p = rng.random(n).astype(np.float32) ** 2
    S = rng.integers(0, 400, n).astype(np.uint32)
    nn = rng.integers(1, 120, n).astype(np.uint32)
    q = (rng.random(n) * 2 - 1).astype(np.float32)
    n_root = (S + rng.integers(0, 3, n)).astype(np.uint32)
    cpuct = 1.0
    # the edge values: p = 0, S = 0, n = 1, n = 0, f_j >= n_j (few visits under a large nf), a prior of exactly 1, 16-bit counts
    p[:400] = 0.0
    S[400:800] = 0
    nn[800:1400] = 1
    nn[1400:1600] = 0
    nn[1600:2400] = rng.integers(1, 4, 800); S[1600:2400] = rng.integers(200, 400, 800); k_e6[1600:2400] = 2000000; p[1600:2400] = np.float32(0.5)
    p[2400:2600] = 1.0
    S[2600:2700] = 7 * 65535; nn[2600:2700] = 65535; n_root[2600:2700] = 65535
    # u*: a random level around the slot's own scores, and -- u* TIES -- exactly the slot's score at some m <= n, where `<` must stop the loop
    sq = np.array([ft.sq_py(int(x)) for x in n_root], np.float32)
    u_star = (rng.random(n) * 3 - 1).astype(np.float32)
    ties = np.arange(3000, 9000)
    for i in ties:
        if nn[i] == 0:
            continue
        m = int(rng.integers(1, int(nn[i]) + 1))
        u_star[i] = ft.puct_py(q[i], m - 1, p[i], sq[i], cpuct)          # q + c / (float)m
    return k_e6, p, S, nn, q, n_root, cpuct, u_star, sq


def test_host_predicates_equal_the_numpy_restatement():
    k_e6, p, S, nn, q, n_root, cpuct, u_star, sq = _cases()
    nf, forced, m, sq_h = ft.host_eval(k_e6, p, S, nn, q, n_root, cpuct, u_star)
    want_nf = np.array([ft.nf_py(int(a), b, int(c)) for a, b, c in zip(k_e6, p, S)], np.float32)
    assert np.array_equal(nf.view(np.uint32), want_nf.view(np.uint32))
    assert np.array_equal(sq_h.view(np.uint32), sq.view(np.uint32))
    want_forced = (nn > 0) & (nn.astype(np.float32) < want_nf)
    assert np.array_equal(forced, want_forced)
    want_m = np.array([ft.prune_py(int(k_e6[i]), p[i], int(S[i]), int(nn[i]), q[i], sq[i], cpuct, u_star[i]) for i in range(len(p))], np.uint32)
    assert np.array_equal(m, want_m)
    # the PUCT restatement of the header against the formula
    pu = ft.host_puct(q, nn, p, n_root, cpuct)
    want_pu = np.array([ft.puct_py(q[i], int(nn[i]), p[i], sq[i], cpuct) for i in range(len(p))], np.float32)
    assert np.array_equal(pu.view(np.uint32), want_pu.view(np.uint32))
    # the cases are not degenerate: every outcome occurs
    lowered = m < nn
    print("forced %d of %d; pruned: unchanged %d, lowered %d, to zero %d, stopped at lo %d" % (
        forced.sum(), len(p), (m == nn).sum(), lowered.sum(), (lowered & (m == 0)).sum(), (lowered & (m > 0)).sum()))
    assert forced.sum() > 1000 and (~forced).sum() > 1000
    assert (m == nn).sum() > 1000 and (lowered & (m == 0)).sum() > 100 and (lowered & (m > 1)).sum() > 1000
    assert not (lowered & (m == 1)).any()                              # the single-playout rule
    assert (k_e6 == 0).sum() > 100 and not forced[k_e6 == 0].any() and np.array_equal(m[k_e6 == 0], nn[k_e6 == 0])    # k = 0: nothing, ever
    assert not forced[:400].any() and not forced[400:800].any()         # p = 0 and S = 0: nf = 0
    # a tie stops the loop: at the tied m the predicate `<` is false, so m never drops below it
    t = np.arange(3000, 9000)
    assert (m[t] > 0).sum() > 1000


# ---- 2. k = 0: the twin is the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
def test_twin_with_k_zero_equals_the_oracle_selfplay(oracle, threads):
    n, sims = 12, 24
    ref = oracle.selfplay(n, sims, net_kind=oracle.NET_HASH, salt=HASH_SALT, seed=11, first_game_id=5, sim_threads=threads)
    for prune in (0, 1):                                                # policy_prune is inert while k = 0
        got = ft.selfplay(n, sims, k=0.0, prune=prune, net_kind=ft.NET_HASH, salt=HASH_SALT, seed=11, first_game_id=5, sim_threads=threads)
        assert got["count"] == ref["count"] == 2 * int(ref["game_len"].sum())
        assert np.array_equal(got["game_len"], ref["game_len"]) and np.array_equal(got["moves"], ref["moves"])
        assert np.array_equal(got["boards"], ref["boards"])
        assert np.array_equal(got["pis"].view(np.uint32), ref["pis"].view(np.uint32)) and np.array_equal(got["zs"], ref["zs"])
        c = got["ctr"]
        assert c["root_sel"] == got["sims"] == sims * int(ref["game_len"].sum())      # the twin's own search copies ran, and forced nothing
        assert c["root_forced"] == 0 and c["moves_pruned"] == 0 and c["moves"] == int(ref["game_len"].sum())


def _c4_play(mine, theirs, a):
    mask = mine | theirs
    nb = (mask + (1 << (a * 7))) & (0x3F << (a * 7))
    return theirs, mine | nb


@pytest.mark.parametrize("threads", [1, 4])
def test_twin_with_k_zero_equals_the_oracle_tree_calls(oracle, threads):
    sims = 48
    for g in range(4):
        tw = ft.Tree(sims, net_kind=ft.NET_HASH, salt=HASH_SALT, threads=threads)
        orc = oracle.Tree(sims, net_kind=oracle.NET_HASH, salt=HASH_SALT, threads=threads)
        s = (0, 0)
        for move in range(6):
            temp = 1.0 if move < 4 else 0.0
            a = tw.get_action_prob(s[0], s[1], temp, 3, 40 + g, k=0.0, prune=1)
            b = orc.get_action_prob(s[0], s[1], temp, seed=3, game_id=40 + g)
            assert np.array_equal(a[0].view(np.uint32), np.asarray(b[0], np.float32).view(np.uint32)), (g, move)
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32))
            s = _c4_play(s[0], s[1], int(np.argmax(a[1])))
        tw.close()
        orc.close()


# ---- 3. the feature does something, and the conditions of the GPU tests hold on their seeds ------------------------------------------------------
@pytest.mark.parametrize("shape", list(GPU_SHAPES))
def test_conditions_hold_for_the_gpu_tests_seeds(shape):
    kw = dict(GPU_SHAPES[shape])
    sims = kw.pop("sims")
    base = ft.selfplay(100, sims, k=0.0, prune=0, net_kind=ft.NET_HASH, salt=GPU_SALT, first_game_id=1000, **kw)
    for prune in (0, 1):
        r = ft.selfplay(100, sims, k=2.0, prune=prune, net_kind=ft.NET_HASH, salt=GPU_SALT, first_game_id=1000, **kw)
        print(shape, "prune", prune)
        check_conditions(r["ctr"], prune, inflight=kw.get("sim_threads", 1) > 1)
        assert not np.array_equal(r["moves"], base["moves"])            # the games really differ from those without the feature
        assert r["sims"] == r["budgets"]
    if "cap_sims" in kw:                                                # composition: both kinds of move occur, only full ones are forced
        full = sum(bin(int(m)).count("1") for m in r["full_masks"])
        assert 0.1 <= full / int(r["game_len"].sum()) <= 0.9
        assert r["ctr"]["moves"] == full and r["ctr"]["root_sel"] == 24 * full


def test_conditions_hold_for_the_tree_call_shape():
    """40 trees, 48 simulations, temperature 1 then 0, k = 2, the same trees called twice per position (S starts non-zero the second time)."""
    for prune in (0, 1):
        for threads in (1, 4):
            ctr = {}
            for g in range(40):
                tw = ft.Tree(48, net_kind=ft.NET_HASH, salt=GPU_SALT, threads=threads)
                for temp in (1.0, 0.0):
                    tw.get_action_prob(0, 0, temp, 3, 40 + g, k=2.0, prune=prune)
                ctr = ft.add_counters(ctr, ft.counters(tw.ctr))
                tw.close()
            check_conditions(ctr, prune, inflight=threads > 1)


def test_pruned_pi_keeps_the_raw_counts_and_moves_mass_to_the_best_child():
    tw0, tw1 = ft.Tree(48, net_kind=ft.NET_HASH, salt=HASH_SALT), ft.Tree(48, net_kind=ft.NET_HASH, salt=HASH_SALT)
    pi0, c0, q0 = tw0.get_action_prob(0, 0, 1.0, 3, 7, k=2.0, prune=0)
    pi1, c1, q1 = tw1.get_action_prob(0, 0, 1.0, 3, 7, k=2.0, prune=1)
    assert np.array_equal(c0, c1) and np.array_equal(q0.view(np.uint32), q1.view(np.uint32))       # the search is the same; counts and q stay raw
    assert int(c0.sum()) == 48
    b = int(np.argmax(c0))
    assert not np.array_equal(pi0, pi1) and pi1[b] > pi0[b]
    assert np.array_equal(pi0, (c0 / np.float32(c0.sum())).astype(np.float32))


# ---- 4. the keys and the hosts ---------------------------------------------------------------------------------------------------------------------
def test_keys_are_documented_and_plumbed(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    host = open(os.path.join(ROOT, "include", "az_host.hpp")).read()
    pysrc = open(os.path.join(ROOT, "alphazero-rs_amd", "engine.py")).read()
    blob = open(engine_mod.LIB_PATH, "rb").read()
    for key in KEYS:
        q = '"%s"' % key
        assert q in hdr and q in md and q in host and q in pysrc, key
        assert key.encode() + b"\0" in blob, key                        # the built library parses the key
    assert "16000000" in hdr and "csrc/az_forced.h" in hdr
    assert hasattr(engine_mod.Engine, "set_forced_playouts") and "set_forced_playouts" in host
    txt = open(os.path.join(ROOT, "alphazero-rs_amd", "csrc", "az_forced.h")).read()
    assert "__builtin_sqrtf" in txt and "__fsqrt_rn(" not in txt and "hip_runtime" not in txt


def test_both_coaches_carry_the_option():
    from alphazero_rs_amd import coach
    src = open(coach.__file__).read()
    host = open(os.path.join(ROOT, "include", "az_host.hpp")).read()
    for text in (src, host):
        assert "forced_playouts_k" in text and "policy_prune" in text

    class Spy:
        def __init__(self):
            self.calls = []

        def set_forced_playouts(self, k, prune=False):
            self.calls.append((k, prune))

    c = coach.Coach.__new__(coach.Coach)
    c.engine, c.forced_playouts_k, c.policy_prune = Spy(), 0.0, True
    with c._selfplay_forced_playouts():
        pass
    assert c.engine.calls == []                                         # k 0: the engine is never asked
    c.forced_playouts_k = 2.0
    with c._selfplay_forced_playouts():
        assert c.engine.calls == [(2.0, True)]
    assert c.engine.calls == [(2.0, True), (0.0, False)]                # on before the episodes, off behind them
