"""Dirichlet root noise on the GPU ("root_noise_eps_e6" / "root_noise_alpha_e6", include/az_engine.h), held to the project's bar: bit-exact
against the twin (tests/cpp/selfplay_twin.cpp -- the unchanged oracle search with the noise restated around it, and the g++ build of the
sampler the kernels compile) on every path a get_action_prob can take, and bit for bit WITHOUT effect where it must have none."""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg        # noqa: E402
import selfplay_twin as tw      # noqa: E402
from feature_gpu import HASH_SALT, c4_play, oracle_salt      # noqa: E402


@pytest.fixture(autouse=True)
def noise_off_afterwards(engine):
    """The session's engine is shared with every other module: leave it as it was found."""
    yield
    fg.restore(engine)


@pytest.fixture(scope="module")
def engine3(engine_mod):
    """The seam's second game (AZ_GAME_CONNECT_THREE)."""
    yield from fg.connect_three_engine(engine_mod)


# ---- 6. options -------------------------------------------------------------------------------------------------------------------------------
def test_option_ranges_and_open_session(engine, engine_mod):
    fg.check_option_ranges(engine, engine_mod,
                           bad=(("root_noise_eps_e6", (-1, 1000001)), ("root_noise_alpha_e6", (0, 49999, 100000001, -5))),
                           good=(("root_noise_eps_e6", (0, 1, 1000000, 250000)), ("root_noise_alpha_e6", (50000, 100000000, 300000))),
                           settle=lambda: engine.set_root_noise(0.0, 1.0),
                           locked=(("root_noise_eps_e6", 250000), ("root_noise_alpha_e6", 300000), ("root_noise_eps_e6", 0)),
                           reopen=("root_noise_eps_e6", 250000))


def _tree_outputs(engine, fused):
    engine.set_option("fused_search", fused)
    tb = engine.tree_create(6, reserve=tw.default_reserve(30), num_sims=30, max_depth=1000, model_id=10, cpuct=1)
    out = []
    states = np.zeros((6, 2), np.uint64)
    for move in range(4):
        pi, counts, q = tb.get_action_prob(states, 1.0 if move < 2 else 0.0, seed=3, first_game_id=40)
        out += [pi, counts, q]
        states = np.array([c4_play(int(s[0]), int(s[1]), int(np.argmax(c))) for s, c in zip(states, counts)], np.uint64)
    tb.close()
    return out


def test_eps_0_set_explicitly_equals_never_set(engine_mod):
    """A fresh engine that never heard of the options against one where eps = 0 was set (after a detour through eps > 0, with another
    alpha left behind): self-play tuples and az_tree_get_action_prob outputs, bit for bit."""
    res = []
    for touch in (False, True):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
        try:
            e.net_set_kind(10, engine_mod.NET_HASH, HASH_SALT)
            if touch:
                e.set_root_noise(0.25, 0.3)
                e.set_option("root_noise_eps_e6", 0)
            sp = e.selfplay(n_games=16, num_sims=25, model_id=10, seed=5, concurrent=8)
            e.set_option("eval_dedup", 2)
            sp2 = e.selfplay(n_games=16, num_sims=25, model_id=10, seed=6)
            e.set_option("eval_dedup", 1)
            res.append([sp[k] for k in ("count", "game_len", "moves", "states", "pis", "zs")] + [sp2[k] for k in ("moves", "pis", "zs")]
                       + _tree_outputs(e, 1) + _tree_outputs(e, 0))
        finally:
            e.close()
    assert len(res[0]) == len(res[1])
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ---- 7. the device sampler against the host build ---------------------------------------------------------------------------------------------
def _random_roots(n, seed):
    """Legal positions of mixed ply, full columns included (random play from the initial board; finished games restart)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 2), np.uint64)
    s, plies = (0, 0), 0
    target = int(rng.integers(0, 40))
    i = 0
    while i < n:
        if plies >= target:
            out[i] = s
            i += 1
            s, plies, target = (0, 0), 0, int(rng.integers(0, 40))
            continue
        # prefer low columns so that some fill up
        legal = [a for a in range(7) if not ((s[0] | s[1]) >> (a * 7 + 5)) & 1]
        if not legal:
            out[i] = s
            i += 1
            s, plies, target = (0, 0), 0, int(rng.integers(0, 40))
            continue
        a = legal[min(int(rng.integers(0, 3)), len(legal) - 1)]
        s = c4_play(s[0], s[1], a)
        plies += 1
    return out


@pytest.mark.parametrize("alpha", [0.05, 0.3, 1.4, 10.0])
def test_device_sampler_matches_the_host_build(engine, alpha):
    n = 4096
    states = _random_roots(n, 5)
    full = [(int(m) | int(t)) for m, t in states]
    assert any(any((f >> (c * 7 + 5)) & 1 for c in range(7)) for f in full), "no partially full board among the roots"
    ids = np.random.default_rng(1).integers(0, 2 ** 63, n).astype(np.uint64)
    engine.set_option("root_noise_alpha_e6", tw.e6(alpha))
    got = engine.root_noise_eta(states, ids, seed=77)
    ref = tw.noise_eta(states, ids, alpha, seed=77)
    bad = np.nonzero((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (alpha, bad[:5], got[bad[:2]], ref[bad[:2]])
    assert np.isfinite(got).all() and np.max(np.abs(got.astype(np.float64).sum(axis=1) - 1)) < 1e-6


# ---- 8. whole-game search parity ----------------------------------------------------------------------------------------------------------------
def play_games_against_twin(engine, oracle, n_games, sims, threads, eps, alpha, seed, game_kind=tw.GAME_BITS, max_moves=42):
    """az_tree_get_action_prob move by move for n_games trees with the twin's trees alongside: pi / counts / q of every move bit-exact.
    Finished games keep searching their last position: that root is then searched AGAIN, and gets the same eta mixed in again on
    both sides (the change is permanent, include/az_engine.h)."""
    engine.set_root_noise(eps, alpha)
    ended = oracle.c3_ended if game_kind == tw.GAME_CONNECT3 else oracle.c4_ended
    tb = engine.tree_create(n_games, reserve=tw.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=10, cpuct=1, num_threads=threads)
    trees = [tw.Tree(sims, net_kind=tw.NET_HASH, salt=oracle_salt(10), model_id=0, game_kind=game_kind, threads=threads) for _ in range(n_games)]
    states, alive = [(0, 0)] * n_games, [True] * n_games
    rng = np.random.default_rng(seed)
    moves = 0
    for move in range(max_moves):
        if not any(alive):
            break
        temp = 1.0 if move < 6 else 0.0
        pi, counts, q = tb.get_action_prob(np.array(states, dtype=np.uint64), temp, seed=seed, first_game_id=100)
        for g in range(n_games):
            opi, ocnt, oq = trees[g].get_action_prob(states[g][0], states[g][1], temp, seed=seed, game_id=100 + g, eps=eps, alpha=alpha)
            assert np.array_equal(counts[g], ocnt), (move, g, counts[g], ocnt)
            assert np.array_equal(pi[g].view(np.uint32), opi.view(np.uint32)), (move, g, pi[g], opi)
            assert np.array_equal(q[g].view(np.uint32), oq.view(np.uint32)), (move, g, q[g], oq)
            if not alive[g]:
                continue
            a = int(rng.choice([a for a in range(7) if opi[a] > 0]))
            nxt = oracle.c4_play(states[g][0], states[g][1], a)
            if ended(*nxt) != 0.0:
                alive[g] = False
            else:
                states[g] = nxt
            moves += 1
    tb.close()
    return moves


@pytest.mark.parametrize("eps,alpha", [(0.25, 0.3), (1.0, 1.4)])
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("fused", [1, 0], ids=["fused-fixture-search", "launch-per-simulation"])
def test_whole_game_search_parity(engine, oracle, fused, threads, eps, alpha):
    engine.set_option("fused_search", fused)
    assert play_games_against_twin(engine, oracle, 6, 24, threads, eps, alpha, seed=11) > 40


@pytest.mark.parametrize("dedup", [0, 1, 2])
def test_whole_game_search_parity_in_every_dedup_mode(engine, oracle, dedup):
    engine.set_option("fused_search", 0)
    engine.set_option("eval_dedup", dedup)
    play_games_against_twin(engine, oracle, 6, 24, 1, 0.25, 0.3, seed=12)


@pytest.mark.parametrize("threads", [1, 4])
def test_whole_game_search_parity_connect_three(engine3, oracle, threads):
    try:
        for fused in (1, 0):
            engine3.set_option("fused_search", fused)
            play_games_against_twin(engine3, oracle, 6, 24, threads, 0.25, 0.3, seed=13, game_kind=tw.GAME_CONNECT3)
    finally:
        engine3.set_option("fused_search", 1)
        engine3.set_root_noise(0.0, 1.0)


# ---- 9. self-play parity --------------------------------------------------------------------------------------------------------------------------
def _check_selfplay(got, ref, symmetries=True):
    fg.check_tuples_against_twin(got, ref, step=1 if symmetries else 2)


SELFPLAY_MODES = {
    "lock-step": dict(),
    "lock-step-per-simulation": dict(options={"fused_search": 0}),
    "async": dict(options={"selfplay_async": 1, "eval_dedup": 2}),
    "async-refill": dict(options={"selfplay_async": 1, "eval_dedup": 2}, concurrent=8),
    "two-sim-threads": dict(num_sim_threads=2, sims=26),
    "two-sim-threads-per-simulation": dict(num_sim_threads=2, sims=26, options={"fused_search": 0}),
    "refill": dict(concurrent=8),
    "refill-dedup": dict(concurrent=8, options={"eval_dedup": 2}),
    "no-symmetries": dict(symmetries=False),
}


@pytest.mark.parametrize("mode", list(SELFPLAY_MODES))
def test_selfplay_parity(engine, mode):
    m = SELFPLAY_MODES[mode]
    n, sims, T = 24, m.get("sims", 25), m.get("num_sim_threads", 1)
    eps, alpha = 0.25, 0.3
    for k, v in m.get("options", {}).items():
        engine.set_option(k, v)
    engine.set_root_noise(eps, alpha)
    got = engine.selfplay(n_games=n, num_sims=sims, model_id=10, seed=21, first_game_id=1000, concurrent=m.get("concurrent", 0),
                          symmetries=m.get("symmetries", True), num_sim_threads=T)
    ref = tw.selfplay(n, sims, net_kind=tw.NET_HASH, salt=oracle_salt(10), seed=21, first_game_id=1000, sim_threads=T, eps=eps, alpha=alpha)
    _check_selfplay(got, ref, m.get("symmetries", True))
    base = tw.selfplay(n, sims, net_kind=tw.NET_HASH, salt=oracle_salt(10), seed=21, first_game_id=1000, sim_threads=T, eps=0.0)
    assert not np.array_equal(base["moves"], ref["moves"])           # the noise really changed the games


@pytest.mark.parametrize("async_mode", [0, 1])
def test_selfplay_session_in_chunks(engine, async_mode):
    n, sims, eps, alpha = 24, 25, 0.25, 1.4
    if async_mode:
        engine.set_option("selfplay_async", 1)
        engine.set_option("eval_dedup", 2)
    engine.set_root_noise(eps, alpha)
    ref = tw.selfplay(n, sims, net_kind=tw.NET_HASH, salt=oracle_salt(10), seed=22, first_game_id=7, eps=eps, alpha=alpha)
    fg.check_session_in_chunks(engine, ref, ((0, 5), (5, 11), (16, 8)),
                               dict(n_games=n, num_sims=sims, model_id=10, seed=22, first_game_id=7, concurrent=8))


# ---- 10. conv-net replay parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [0, 1], ids=["bf16", "fp8"])
def test_conv_net_replay_parity(engine_mod, fp8):
    """Self-play with the conv net and record_evals; the log is fed to the twin's ReplayNet: identical games.  The recorded (pi, v) rows
    are the RAW net outputs (noise never reaches the log, the cache or the de-duplication), and the cache accounting stays consistent."""
    e = engine_mod.Engine(device=0, max_batch=64, net_channels=128)
    try:
        e.net_init_random(0, seed=3)
        if fp8:
            e.set_option("net_fp8", 1)
        n, sims, cap, eps, alpha = 8, 25, 42 * 26 + 8, 0.25, 0.3
        for async_mode in ((0, 1) if not fp8 else (0,)):
            e.set_option("selfplay_async", async_mode)
            e.set_root_noise(eps, alpha)
            e.reset_stats()
            got = e.selfplay(n_games=n, num_sims=sims, model_id=0, seed=9, record_evals=cap)
            cnt, states, pis, vs = e.selfplay_get_evals(n, cap)
            off, fs, fp, fv = fg.flatten_eval_log(cnt, states, pis, vs)
            ref = tw.selfplay(n, sims, net_kind=tw.NET_REPLAY, seed=9, replay=(off, fs, fp, fv), eps=eps, alpha=alpha)
            assert not ref["replay_bad"].any()
            _check_selfplay(got, ref)
            pi2, v2 = e.predict_states(fs[:64], 0)
            assert np.array_equal(pi2, fp[:64]) and np.array_equal(v2, fv[:64])
            st = e.stats()
            assert st["leaf_rows_requested"] == st["leaf_rows_executed"] + st["eval_cache_hits"] + st["eval_batch_dups"], st
            plain = tw.selfplay(n, sims, net_kind=tw.NET_REPLAY, seed=9, replay=(off, fs, fp, fv), eps=0.0)
            assert plain["replay_bad"].any() or not np.array_equal(plain["moves"], ref["moves"])     # the log is a NOISY game's log
    finally:
        e.close()


# ---- 11. shared slots ---------------------------------------------------------------------------------------------------------------------------------
def test_shared_slots_equal_one_game_trees(engine):
    """Four host threads, one slot each, their own (seed, game_id) streams: every answer equals the 1-game tree's for the same
    (seed, game_id, state) sequence."""
    sims, eps, alpha, moves = 25, 0.25, 0.3, 6
    engine.set_root_noise(eps, alpha)
    streams = [(31, 5), (31, 6), (99, 5), (7, 123456789)]
    want = []
    for seed, gid in streams:
        tb = engine.tree_create(1, reserve=tw.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=10, cpuct=1)
        s, seq = (0, 0), []
        for move in range(moves):
            pi, counts, q = tb.get_action_prob(np.array([s], np.uint64), 1.0 if move < 3 else 0.0, seed=seed, first_game_id=gid)
            seq.append((pi[0].copy(), counts[0].copy(), q[0].copy()))
            s = c4_play(s[0], s[1], int(np.argmax(counts[0])))
        tb.close()
        want.append(seq)
    assert not np.array_equal(want[0][0][1], want[1][0][1]) or not np.array_equal(want[0][0][2], want[1][0][2])   # streams differ
    shared = engine.tree_create(4, reserve=tw.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=10, cpuct=1)
    shared.share(0)
    got, errs = [None] * 4, []

    def worker(i):
        try:
            slot = shared.slot_acquire()
            start.wait()
            seed, gid = streams[i]
            s, seq = (0, 0), []
            for move in range(moves):
                pi, counts, q = shared.slot_get_action_prob(slot, s, 1.0 if move < 3 else 0.0, seed=seed, game_id=gid)
                seq.append((pi, counts, q))
                s = c4_play(s[0], s[1], int(np.argmax(counts)))
            got[i] = seq
            shared.slot_release(slot)
        except Exception as ex:      # noqa: BLE001
            errs.append(repr(ex))

    start = threading.Barrier(4)
    th = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs and all(not t.is_alive() for t in th), errs
    shared.close()
    for i in range(4):
        for a, b in zip(got[i], want[i]):
            for x, y in zip(a, b):
                assert np.array_equal(x, y), i


# ---- 12. the arena never sees it ------------------------------------------------------------------------------------------------------------------------
def test_arena_is_noise_free(engine):
    engine.set_root_noise(0.0, 1.0)
    want = fg.arena_outputs(engine)
    engine.set_root_noise(1.0, 0.3)
    engine.selfplay(n_games=8, num_sims=25, model_id=10, seed=1)          # leaves a noisy arena behind in the pool
    fg.assert_same_outputs(fg.arena_outputs(engine), want)


# ---- 13. the two Coaches ----------------------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_coach_agree_with_root_noise(engine_mod, tmp_path):
    """tests/test_coach_gpu.py::test_python_and_cpp_coach_agree with Coach.root_noise_eps / root_noise_alpha set on both hosts:
    byte-identical files, and different ones from the noise-free run's."""
    def noise(eps):
        def configure(coach, e):
            coach.root_noise_eps, coach.root_noise_alpha = eps, 0.3
        return configure
    fg.run_coach_pair(engine_mod, tmp_path, ["root_noise_eps=0.25", "root_noise_alpha=0.3"], noise(0.25), plain=noise(0.0))
