"""Forced playouts and policy target pruning on the GPU ("forced_playouts_k_e6" / "policy_prune", include/az_engine.h), held to the
project's bar: bit-exact against the twin (tests/cpp/selfplay_twin.cpp -- the unchanged oracle with the feature restated around it, and the
g++ build of the predicates the kernels compile) on every path a forced move can take, and bit for bit WITHOUT effect where it must have
none.

Shapes follow tests/test_playout_cap_gpu.py: 100 episodes on 40 slots = one whole 256-lane tree workgroup (32 games) plus one partial
wave, with slot refill; the hash net as model 10.  24 simulations (fused, de-duplicated, four simulation threads, free-running), 44 where
the search crosses a 20-step graph chunk, 25 on Connect Three; tree calls at 48.  Every parity test asserts on the twin's counters that at
least 5 % of the root selections it compared were decided by a forced child, with several simulations in flight that one of them was made
while earlier simulations of its step were in flight, and with pruning on that the pruned counts differ from the raw ones on at least
half of the moves and that a child went from two or more visits to none by the single-playout rule
(tests/test_forced_playouts_cpu.py asserts the same on the CPU alone for these seeds)."""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg        # noqa: E402
import selfplay_twin as ft      # noqa: E402
from feature_gpu import COUNTERS, HASH_SALT, N_GAMES, PER_SIM, SLOTS, c4_play, oracle_salt      # noqa: E402

K = 2.0


@pytest.fixture(autouse=True)
def forced_off_afterwards(engine):
    """The session's engine is shared with every other module: leave it as it was found."""
    yield
    fg.restore(engine)


@pytest.fixture(scope="module")
def engine3(engine_mod):
    """The seam's second game (AZ_GAME_CONNECT_THREE)."""
    yield from fg.connect_three_engine(engine_mod)


def check_conditions(ctr, prune, inflight=False):
    """Conditions, not measurements: the parity above compared forced selections and pruned targets, not a search that never met either."""
    print({k: ctr[k] for k in ft.COUNTERS})
    assert ctr["root_sel"] > 0 and ctr["root_forced"] >= 0.05 * ctr["root_sel"], ctr
    if inflight:
        assert ctr["root_forced_inflight"] >= 1, ctr
    if prune:
        assert ctr["moves"] > 0 and ctr["moves_pruned"] >= 0.5 * ctr["moves"], ctr
        assert ctr["to_zero"] >= 1, ctr


def forced_selfplay(e, sims, k, prune, seed, **kw):
    return fg.run_selfplay(e, sims, seed, forced=(k, prune), **kw)


def check_against_twin(got, ref, prune, inflight=False):
    fg.check_samples_against_twin(got, ref)
    check_conditions(ref["ctr"], prune, inflight)


# ---- options ------------------------------------------------------------------------------------------------------------------------------
def test_option_ranges_and_open_session(engine, engine_mod):
    fg.check_option_ranges(engine, engine_mod,
                           bad=(("forced_playouts_k_e6", (-1, 16000001, 1 << 40)), ("policy_prune", (-1, 2, 1000000))),
                           good=(("forced_playouts_k_e6", (0, 1, 16000000, 2000000)), ("policy_prune", (0, 1))),
                           settle=lambda: engine.set_forced_playouts(0.0, False),
                           locked=(("forced_playouts_k_e6", 2000000), ("policy_prune", 1), ("forced_playouts_k_e6", 0), ("policy_prune", 0)),
                           reopen=("forced_playouts_k_e6", 2000000))


# ---- off means off ----------------------------------------------------------------------------------------------------------------------------
OFF_RUNS = [dict(options={}, concurrent=SLOTS), dict(options={"selfplay_async": 1, "eval_dedup": 2}, concurrent=SLOTS),
            dict(options={"fused_search": 0}, concurrent=0, threads=4)]


def _off_outputs(e, touch):
    out = []
    for run in OFF_RUNS:
        for key, v in (("selfplay_async", 0), ("eval_dedup", 1), ("fused_search", 1)):
            e.set_option(key, v)
        for key, v in run["options"].items():
            e.set_option(key, v)
        if touch:
            e.set_option("policy_prune", 1)
            e.set_option("forced_playouts_k_e6", 0)
        e.reset_stats()
        got = e.selfplay(n_games=N_GAMES, num_sims=24, model_id=10, seed=11, first_game_id=1000, concurrent=run["concurrent"],
                         num_sim_threads=run.get("threads", 1))
        got["stats"] = e.stats()
        out.append(got)
    for key, v in (("selfplay_async", 0), ("eval_dedup", 1), ("fused_search", 1)):
        e.set_option(key, v)
    e.reset_stats()
    other = fg.other_entry_points(e)
    return out, other, e.stats()


def test_off_equals_never_set(engine_mod):
    """A fresh engine that never heard of the keys against one with k = 0 and policy_prune = 1: self-play (lock-step, free-running, four
    simulation threads), tree call, slot call, arena, and every counter."""
    res = []
    for touch in (False, True):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
        try:
            e.net_set_kind(10, engine_mod.NET_HASH, HASH_SALT)
            e.net_set_kind(11, engine_mod.NET_HASH, HASH_SALT)
            res.append(_off_outputs(e, touch))
        finally:
            e.close()
    (sp_a, other_a, st_a), (sp_b, other_b, st_b) = res
    for a, b in zip(sp_a, sp_b):
        for key in ("count", "game_len", "moves", "states", "boards", "pis", "zs"):
            assert np.array_equal(a[key], b[key]), key
        for key in COUNTERS:
            assert a["stats"][key] == b["stats"][key], (key, a["stats"][key], b["stats"][key])
    fg.assert_same_outputs(other_a, other_b)
    for key in COUNTERS:
        assert st_a[key] == st_b[key], key


# ---- tree calls ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("prune", [0, 1])
def test_tree_call_parity(engine, prune, threads):
    """az_tree_get_action_prob on 40 trees, 48 simulations: temperature 1, the SAME roots a second time at temperature 0 (persistent tree:
    S starts non-zero), then the position after the most visited move."""
    G, sims = 40, 48
    engine.set_forced_playouts(K, prune)
    tb = engine.tree_create(G, reserve=ft.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=10, cpuct=1, num_threads=threads)
    twins = [ft.Tree(sims, net_kind=ft.NET_HASH, salt=oracle_salt(10), threads=threads) for _ in range(G)]
    try:
        states = np.zeros((G, 2), np.uint64)
        ctr = {}
        for call, temp in enumerate((1.0, 0.0, 1.0, 0.0)):
            pi, counts, q = tb.get_action_prob(states, temp, seed=3, first_game_id=40)
            for g in range(G):
                rpi, rc, rq = twins[g].get_action_prob(int(states[g, 0]), int(states[g, 1]), temp, 3, 40 + g, k=K, prune=prune)
                assert np.array_equal(counts[g], rc), (call, g, counts[g], rc)                      # raw
                assert np.array_equal(q[g].view(np.uint32), rq.view(np.uint32)), (call, g)
                assert np.array_equal(pi[g].view(np.uint32), rpi.view(np.uint32)), (call, g, pi[g], rpi)
            if call == 0:
                assert (counts.sum(axis=1) == sims).all()
                if prune:       # pi is NOT the raw counts' on most trees, and sums to 1
                    raw = (counts / np.float32(sims)).astype(np.float32)
                    assert (np.abs(pi - raw).max(axis=1) > 0).mean() >= 0.5
                    assert np.allclose(pi.sum(axis=1), 1.0, atol=1e-6)
            if call == 1:
                states = np.array([c4_play(int(s[0]), int(s[1]), int(np.argmax(c))) for s, c in zip(states, counts)], np.uint64)
        for t in twins:
            ctr = ft.add_counters(ctr, ft.counters(t.ctr))
        check_conditions(ctr, prune, inflight=threads > 1)
    finally:
        tb.close()
        for t in twins:
            t.close()


@pytest.mark.parametrize("prune", [0, 1])
def test_slot_call_parity(engine, prune):
    """az_tree_slot_get_action_prob: 40 host threads with one slot of a shared batch each (a batch coalesces the holders' requests), each
    on its own stream, twice on the same root and once a move later."""
    G, sims = 40, 48
    engine.set_forced_playouts(K, prune)
    shared = engine.tree_create(G, reserve=ft.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=10, cpuct=1)
    shared.share(0)
    got, errs = [None] * G, []
    start = threading.Barrier(G)

    def worker(g):
        try:
            slot = shared.slot_acquire()
            start.wait()
            s, seq = (0, 0), []
            for call, temp in enumerate((1.0, 0.0, 1.0)):
                pi, counts, q = shared.slot_get_action_prob(slot, s, temp, seed=31, game_id=500 + g)
                seq.append((s, temp, pi, counts, q))
                if call == 1:
                    s = c4_play(s[0], s[1], int(np.argmax(counts)))
            got[g] = seq
            shared.slot_release(slot)
        except Exception as ex:      # noqa: BLE001
            errs.append(repr(ex))

    th = [threading.Thread(target=worker, args=(g,), daemon=True) for g in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not errs and all(not t.is_alive() for t in th), errs
    shared.close()
    ctr = {}
    for g in range(G):
        tw = ft.Tree(sims, net_kind=ft.NET_HASH, salt=oracle_salt(10))
        for call, (s, temp, pi, counts, q) in enumerate(got[g]):
            rpi, rc, rq = tw.get_action_prob(s[0], s[1], temp, 31, 500 + g, k=K, prune=prune)
            assert np.array_equal(counts, rc) and np.array_equal(q.view(np.uint32), rq.view(np.uint32)), (g, call)
            assert np.array_equal(pi.view(np.uint32), rpi.view(np.uint32)), (g, call, pi, rpi)
        ctr = ft.add_counters(ctr, ft.counters(tw.ctr))
        tw.close()
    check_conditions(ctr, prune)


# ---- self-play parity against the twin ------------------------------------------------------------------------------------------------------------
MODES = {
    # name: (options, threads, sims, seed)
    "fused-24": ({}, 1, 24, 11),
    "per-simulation-graph-44": (PER_SIM, 1, 44, 12),
    "dedup-2-24": (dict(PER_SIM, eval_dedup=2), 1, 24, 12),
    "four-sim-threads-24": ({}, 4, 24, 11),
    "four-sim-threads-per-simulation-24": (PER_SIM, 4, 24, 12),
    "async-24": ({"selfplay_async": 1, "eval_dedup": 2}, 1, 24, 12),
}


@pytest.mark.parametrize("prune", [0, 1])
@pytest.mark.parametrize("mode", list(MODES))
def test_selfplay_parity(engine, mode, prune):
    options, threads, sims, seed = MODES[mode]
    got = forced_selfplay(engine, sims, K, prune, seed, threads=threads, options=options)
    ref = ft.selfplay(N_GAMES, sims, k=K, prune=prune, net_kind=ft.NET_HASH, salt=oracle_salt(10), seed=seed, first_game_id=1000, sim_threads=threads)
    check_against_twin(got, ref, prune, inflight=threads > 1)


@pytest.mark.parametrize("mode", ["fused", "per-simulation", "async"])
def test_selfplay_parity_connect_three(engine3, mode):
    options = {"fused": {}, "per-simulation": PER_SIM, "async": {"selfplay_async": 1, "eval_dedup": 2}}[mode]
    try:
        got = forced_selfplay(engine3, 25, K, 1, 12, options=options)
        ref = ft.selfplay(N_GAMES, 25, k=K, prune=1, net_kind=ft.NET_HASH, salt=oracle_salt(10), seed=12, first_game_id=1000, game_kind=ft.GAME_CONNECT3)
        check_against_twin(got, ref, 1)
    finally:
        fg.restore(engine3)


@pytest.mark.parametrize("mode", ["lock-step", "per-simulation", "async", "four-sim-threads"])
def test_composition_with_root_noise_and_playout_cap(engine, mode):
    """Root noise 0.25 + playout cap (24, 8, P = 0.5) + forced playouts + pruning: full moves are forced and noisy, fast moves neither."""
    options = {"lock-step": {}, "per-simulation": PER_SIM, "async": {"selfplay_async": 1, "eval_dedup": 2}, "four-sim-threads": {}}[mode]
    threads = 4 if mode == "four-sim-threads" else 1
    got = forced_selfplay(engine, 24, K, 1, 11, threads=threads, options=options, cap=(8, 500000), noise=(0.25, 0.3))
    kw = dict(net_kind=ft.NET_HASH, salt=oracle_salt(10), seed=11, first_game_id=1000, sim_threads=threads, cap_sims=8, full_e6=500000, eps=0.25, alpha=0.3)
    ref = ft.selfplay(N_GAMES, 24, k=K, prune=1, **kw)
    check_against_twin(got, ref, 1, inflight=threads > 1)
    full, plies = sum(bin(int(m)).count("1") for m in ref["full_masks"]), int(ref["game_len"].sum())
    assert 0.1 <= full / plies <= 0.9
    assert ref["ctr"]["moves"] == full and ref["ctr"]["root_sel"] == 24 * full          # only the full moves were forced moves
    plain = ft.selfplay(N_GAMES, 24, k=0.0, prune=0, **kw)
    assert not np.array_equal(plain["moves"], ref["moves"])              # the feature really changed the games


# ---- a session fetched in chunks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("async_mode", [0, 1])
def test_session_in_chunks_equals_one_call(engine, async_mode):
    options = {"selfplay_async": 1, "eval_dedup": 2} if async_mode else PER_SIM
    sims, seed = 44, 12
    one = forced_selfplay(engine, sims, K, 1, seed, options=options)
    ref = ft.selfplay(N_GAMES, sims, k=K, prune=1, net_kind=ft.NET_HASH, salt=oracle_salt(10), seed=seed, first_game_id=1000)
    check_against_twin(one, ref, 1)
    fg.check_session_in_chunks(engine, one, ((0, 30), (30, 30), (60, 40)),
                               dict(n_games=N_GAMES, num_sims=sims, model_id=10, seed=seed, first_game_id=1000, concurrent=SLOTS))


# ---- conv-net replay parity ---------------------------------------------------------------------------------------------------------------------------
def test_conv_net_replay_parity(engine_mod):
    """Self-play with the conv net (C = 128) and record_evals; the log is fed to the twin's ReplayNet, which must consume every record of
    every episode exactly.  A randomly initialised conv net has near-uniform priors and near-constant values, so its searches spread
    their visits evenly and at k = 2 pruning alters few targets (the twin, on this net: 17 % of the moves at 24 simulations, 33 % at 48,
    with or without root noise -- below the module's 50 % condition).  The shape is therefore 48 simulations with root noise 0.25 and
    k = 8, where the twin prunes the target of 94 % of the moves and 93 % of the root selections are forced."""
    e = engine_mod.Engine(device=0, max_batch=64, net_channels=128)
    try:
        e.net_init_random(0, seed=3)
        sims, seed, k, noise = 48, 12, 8.0, (0.25, 0.3)
        cap = 42 * (sims + 1) + 8
        got = forced_selfplay(e, sims, k, 1, seed, model_id=0, record_evals=cap, noise=noise)
        cnt, states, pis, vs = e.selfplay_get_evals(N_GAMES, cap)
        assert (cnt > 0).all() and (cnt < cap).all()
        ref = ft.selfplay(N_GAMES, sims, k=k, prune=1, net_kind=ft.NET_REPLAY, seed=seed, first_game_id=1000,
                          replay=fg.flatten_eval_log(cnt, states, pis, vs), eps=noise[0], alpha=noise[1])
        assert not ref["replay_bad"].any()
        check_against_twin(got, ref, 1)
        st = got["stats"]
        assert st["leaf_rows_requested"] == st["leaf_rows_executed"] + st["eval_cache_hits"] + st["eval_batch_dups"], st
    finally:
        e.close()


# ---- the arena never sees it ---------------------------------------------------------------------------------------------------------------------------
def test_arena_ignores_the_keys(engine):
    want = fg.arena_outputs(engine)
    forced_selfplay(engine, 24, K, 1, 11, n_games=16, concurrent=8)     # leaves a forced arena behind in the pool; the keys stay set
    fg.assert_same_outputs(fg.arena_outputs(engine), want)


# ---- the two Coaches ------------------------------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_coach_agree_with_forced_playouts(engine_mod, tmp_path):
    """tests/test_coach_gpu.py::test_python_and_cpp_coach_agree with Coach.forced_playouts_k / policy_prune (and root noise) set on both
    hosts: byte-identical files; the option is on for the episodes and off again behind them."""
    seen = []

    def configure(coach, e):
        coach.root_noise_eps, coach.root_noise_alpha = 0.25, 0.3
        coach.forced_playouts_k, coach.policy_prune = K, True
        orig = e.set_option

        def spy(key, value):
            if key in ("forced_playouts_k_e6", "policy_prune"):
                seen.append((key, value))
            return orig(key, value)
        e.set_option = spy
    fg.run_coach_pair(engine_mod, tmp_path, ["root_noise_eps=0.25", "root_noise_alpha=0.3", "forced_playouts_k=2.0", "policy_prune=1"], configure)
    assert seen == [("policy_prune", 1), ("forced_playouts_k_e6", 2000000), ("policy_prune", 0), ("forced_playouts_k_e6", 0)], seen
