"""Playout cap randomization on the GPU ("playout_cap_sims" / "playout_cap_full_e6", include/az_engine.h), held to the project's bar:
bit-exact against the twin (tests/cpp/selfplay_twin.cpp -- the unchanged oracle with the feature restated around it, and the g++
build of the predicate the kernels compile) on every path a self-play move can take, and bit for bit WITHOUT effect where it must have
none.

Shapes: 100 episodes on 40 slots = one whole 256-lane tree workgroup (32 games) plus one partial wave, with slot refill.  (N, n) =
(24, 8) with one and four simulation threads; (44, 12), where a fast budget ends inside the first replayed 20-step graph chunk and a full
one after two chunks and a remainder; (25, 5) on Connect Three.  Every parity test asserts that between 10 % and 90 % of the plies it
compared were full moves and that both kinds occur at ply 0 (seeds 11 / 12, P = 0.25 / 0.5: tests/test_playout_cap_cpu.py)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg        # noqa: E402
import selfplay_twin as pc      # noqa: E402
from feature_gpu import AZ_ERR_BAD_ARGUMENT, COUNTERS, HASH_SALT, N_GAMES, PER_SIM, SLOTS, oracle_salt      # noqa: E402


@pytest.fixture(autouse=True)
def cap_off_afterwards(engine):
    """The session's engine is shared with every other module: leave it as it was found."""
    yield
    fg.restore(engine)


@pytest.fixture(scope="module")
def engine3(engine_mod):
    """The seam's second game (AZ_GAME_CONNECT_THREE)."""
    yield from fg.connect_three_engine(engine_mod)


def capped_selfplay(e, sims, cap_sims, full_e6, seed, **kw):
    return fg.run_selfplay(e, sims, seed, cap=(cap_sims, full_e6), **kw)


def check_against_twin(got, ref, degenerate_ok=False):
    full, plies = fg.check_samples_against_twin(got, ref)
    if not degenerate_ok:
        assert 0.1 <= full / plies <= 0.9, (full, plies)
        first = sum(int(m) & 1 for m in ref["full_masks"])
        assert 0 < first < len(ref["full_masks"]), first


# ---- options ------------------------------------------------------------------------------------------------------------------------------
def test_option_ranges_and_open_session(engine, engine_mod):
    fg.check_option_ranges(engine, engine_mod,
                           bad=(("playout_cap_sims", (-1, 65536, 1 << 40)), ("playout_cap_full_e6", (-1, 1000001))),
                           good=(("playout_cap_sims", (0, 1, 65535, 8)), ("playout_cap_full_e6", (0, 1, 1000000, 250000))),
                           settle=lambda: engine.set_option("playout_cap_sims", 0),
                           locked=(("playout_cap_sims", 5), ("playout_cap_full_e6", 500000), ("playout_cap_sims", 0)),
                           reopen=("playout_cap_sims", 5))


def test_refusals_at_begin(engine, engine_mod):
    for cap_sims, sims, threads in ((24, 24, 1), (30, 24, 1), (6, 24, 4)):
        engine.set_option("playout_cap_sims", cap_sims)
        for call in ("selfplay", "begin"):
            with pytest.raises(engine_mod.AzError) as ei:
                if call == "selfplay":
                    engine.selfplay(n_games=4, num_sims=sims, model_id=10, seed=1, num_sim_threads=threads)
                else:
                    engine.selfplay_begin(4, sims, 10, seed=1, num_sim_threads=threads)
            assert ei.value.status == AZ_ERR_BAD_ARGUMENT and "playout_cap_sims" in str(ei.value), (cap_sims, sims, threads, str(ei.value))
    engine.set_option("playout_cap_sims", 8)            # a legal pair right behind the refusals
    engine.selfplay(n_games=4, num_sims=24, model_id=10, seed=1, num_sim_threads=4)


# ---- off means off ----------------------------------------------------------------------------------------------------------------------------
OFF_RUNS = [dict(options={}, concurrent=SLOTS), dict(options={}, concurrent=0),
            dict(options={"selfplay_async": 1, "eval_dedup": 2}, concurrent=SLOTS), dict(options={"selfplay_async": 1, "eval_dedup": 2}, concurrent=0)]


def _off_outputs(e, cap_sims, full_e6, touch):
    out = []
    for run in OFF_RUNS:
        e.set_option("selfplay_async", 0)
        e.set_option("eval_dedup", 1)
        if touch:
            got = capped_selfplay(e, 24, cap_sims, full_e6, seed=11, **run)
        else:
            for k, v in run["options"].items():
                e.set_option(k, v)
            e.reset_stats()
            got = e.selfplay(n_games=N_GAMES, num_sims=24, model_id=10, seed=11, first_game_id=1000, concurrent=run["concurrent"])
            got["full_masks"], got["stats"] = e.selfplay_full_plies(), e.stats()
        out.append(got)
    return out


def test_off_and_every_move_full_equal_never_set(engine_mod):
    """A fresh engine that never heard of the keys against one with n = 0 and some P, and against one with n > 0 and P = 1000000:
    samples, game_len, moves, masks and the stats counters, lock-step and free-running, with and without slot refill."""
    res = []
    for cap_sims, full_e6, touch in ((0, 0, False), (0, 123456, True), (8, 1000000, True)):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
        try:
            e.net_set_kind(10, engine_mod.NET_HASH, HASH_SALT)
            res.append(_off_outputs(e, cap_sims, full_e6, touch))
        finally:
            e.close()
    for other in res[1:]:
        for a, b in zip(res[0], other):
            for k in ("count", "game_len", "moves", "states", "boards", "pis", "zs", "full_masks"):
                assert np.array_equal(a[k], b[k]), k
            assert [int(m) for m in a["full_masks"]] == [(1 << int(l)) - 1 for l in a["game_len"]]
            for k in COUNTERS:
                assert a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])


# ---- self-play parity against the twin ------------------------------------------------------------------------------------------------------------
MODES = {
    # name: (options, threads, (N, n), P, seed)
    "lock-step-fused-24-8": ({}, 1, (24, 8), 250000, 11),
    "lock-step-fused-44-12": ({}, 1, (44, 12), 500000, 12),
    "per-simulation-24-8": (PER_SIM, 1, (24, 8), 500000, 12),
    "per-simulation-graph-44-12": (PER_SIM, 1, (44, 12), 250000, 11),
    "dedup-0-24-8": (dict(PER_SIM, eval_dedup=0), 1, (24, 8), 250000, 12),
    "dedup-1-44-12": (dict(PER_SIM, eval_dedup=1), 1, (44, 12), 500000, 11),
    "dedup-2-24-8": (dict(PER_SIM, eval_dedup=2), 1, (24, 8), 500000, 11),
    "dedup-2-graph-44-12": (dict(PER_SIM, eval_dedup=2), 1, (44, 12), 250000, 12),
    "four-sim-threads-24-8": ({}, 4, (24, 8), 250000, 11),
    "four-sim-threads-dedup-2-24-8": (dict(PER_SIM, eval_dedup=2), 4, (24, 8), 500000, 12),
    "async-24-8": ({"selfplay_async": 1, "eval_dedup": 2}, 1, (24, 8), 250000, 11),
    "async-44-12": ({"selfplay_async": 1, "eval_dedup": 2}, 1, (44, 12), 500000, 12),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_selfplay_parity(engine, mode):
    options, threads, (sims, cap_sims), full_e6, seed = MODES[mode]
    got = capped_selfplay(engine, sims, cap_sims, full_e6, seed, threads=threads, options=options)
    ref = pc.selfplay(N_GAMES, sims, cap_sims=cap_sims, full_e6=full_e6, net_kind=pc.NET_HASH, salt=oracle_salt(10), seed=seed, first_game_id=1000, sim_threads=threads)
    check_against_twin(got, ref)


@pytest.mark.parametrize("mode", ["fused", "per-simulation", "async"])
def test_selfplay_parity_connect_three(engine3, mode):
    options = {"fused": {}, "per-simulation": PER_SIM, "async": {"selfplay_async": 1, "eval_dedup": 2}}[mode]
    try:
        got = capped_selfplay(engine3, 25, 5, 500000, 12, options=options)
        ref = pc.selfplay(N_GAMES, 25, cap_sims=5, full_e6=500000, net_kind=pc.NET_HASH, salt=oracle_salt(10), seed=12, first_game_id=1000, game_kind=pc.GAME_CONNECT3)
        check_against_twin(got, ref)
    finally:
        fg.restore(engine3)


@pytest.mark.parametrize("mode", ["lock-step-fused-24-8", "per-simulation-graph-44-12", "dedup-2-24-8", "four-sim-threads-24-8",
                                  "four-sim-threads-dedup-2-24-8", "async-44-12"])
def test_selfplay_parity_with_root_noise(engine, mode):
    """Full moves are noisy, fast moves are not."""
    options, threads, (sims, cap_sims), full_e6, seed = MODES[mode]
    engine.set_root_noise(0.25, 0.3)
    got = capped_selfplay(engine, sims, cap_sims, full_e6, seed, threads=threads, options=options)
    kw = dict(net_kind=pc.NET_HASH, salt=oracle_salt(10), seed=seed, first_game_id=1000, sim_threads=threads)
    ref = pc.selfplay(N_GAMES, sims, cap_sims=cap_sims, full_e6=full_e6, eps=0.25, alpha=0.3, **kw)
    check_against_twin(got, ref)
    plain = pc.selfplay(N_GAMES, sims, cap_sims=cap_sims, full_e6=full_e6, **kw)
    assert not np.array_equal(plain["moves"], ref["moves"])              # the noise really changed the games


def test_no_full_move_emits_no_tuple(engine):
    got = capped_selfplay(engine, 24, 8, 0, 11)
    ref = pc.selfplay(N_GAMES, 24, cap_sims=8, full_e6=0, net_kind=pc.NET_HASH, salt=oracle_salt(10), seed=11, first_game_id=1000)
    assert got["count"] == 0 and not got["full_masks"].any()
    check_against_twin(got, ref, degenerate_ok=True)


# ---- a session fetched in chunks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("async_mode", [0, 1])
def test_session_in_chunks_equals_one_call(engine, async_mode):
    options = {"selfplay_async": 1, "eval_dedup": 2} if async_mode else PER_SIM
    sims, cap_sims, full_e6, seed = 44, 12, 250000, 11
    one = capped_selfplay(engine, sims, cap_sims, full_e6, seed, options=options)
    assert 0.1 <= pc.popcount(one["full_masks"]) / int(one["game_len"].sum()) <= 0.9
    fg.check_session_in_chunks(engine, one, ((0, 30), (30, 30), (60, 40)),
                               dict(n_games=N_GAMES, num_sims=sims, model_id=10, seed=seed, first_game_id=1000, concurrent=SLOTS))


# ---- conv-net replay parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("klass", ["bf16", "fp8-mirror"])
def test_conv_net_replay_parity(engine_mod, klass):
    """Self-play with the conv net and record_evals; the log is fed to the twin's ReplayNet, which must consume every record of every
    episode exactly -- the log holds every predict of the episode, fast moves included."""
    e = engine_mod.Engine(device=0, max_batch=64, net_channels=128)
    try:
        e.net_init_random(0, seed=3)
        if klass != "bf16":
            e.set_option("net_fp8", 1)
            e.set_eval_mirror(1)
        sims, cap_sims, full_e6, seed = 24, 8, 500000, 12
        cap = 42 * (sims + 1) + 8
        for async_mode in ((0, 1) if klass == "bf16" else (0,)):
            got = capped_selfplay(e, sims, cap_sims, full_e6, seed, options={"selfplay_async": async_mode}, model_id=0, record_evals=cap)
            cnt, states, pis, vs = e.selfplay_get_evals(N_GAMES, cap)
            assert (cnt > 0).all() and (cnt < cap).all()
            ref = pc.selfplay(N_GAMES, sims, cap_sims=cap_sims, full_e6=full_e6, net_kind=pc.NET_REPLAY, seed=seed, first_game_id=1000,
                              replay=fg.flatten_eval_log(cnt, states, pis, vs))
            assert not ref["replay_bad"].any()
            check_against_twin(got, ref)
            st = got["stats"]
            assert st["leaf_rows_requested"] == st["leaf_rows_executed"] + st["eval_cache_hits"] + st["eval_batch_dups"], st
    finally:
        e.close()


# ---- the arena and the tree calls never see it --------------------------------------------------------------------------------------------------------------
def test_arena_and_tree_calls_ignore_the_keys(engine):
    want = fg.other_entry_points(engine)
    capped_selfplay(engine, 24, 8, 250000, 11, n_games=16, concurrent=8)     # leaves a capped arena behind in the pool; the keys stay set
    fg.assert_same_outputs(fg.other_entry_points(engine), want)


# ---- the two Coaches ------------------------------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_coach_agree_with_a_playout_cap(engine_mod, tmp_path):
    """tests/test_coach_gpu.py::test_python_and_cpp_coach_agree with Coach.playout_cap_sims / playout_cap_full set on both hosts:
    byte-identical files, written from the full moves only."""
    seen = []

    def configure(coach, e):
        coach.playout_cap_sims, coach.playout_cap_full = 5, 0.5
        orig = e.selfplay

        def spy(**kw):
            r = orig(**kw)
            seen.append((int(r["game_len"].sum()), r["count"], pc.popcount(e.selfplay_full_plies())))
            return r
        e.selfplay = spy

    def inspect(e):
        del e.selfplay                                   # the spy: the class's method again
        e.selfplay(n_games=2, num_sims=25, model_id=0, seed=1)
        assert int(e.selfplay_full_plies()[0]) & 1 and e.stats()["samples"] > 0     # cleared behind the episodes: every ply is recorded again
    fg.run_coach_pair(engine_mod, tmp_path, ["playout_cap_sims=5", "playout_cap_full=0.5"], configure, inspect=inspect)
    assert len(seen) == 1 and seen[0][1] == seen[0][2] and 0.1 * seen[0][0] <= seen[0][1] <= 0.9 * seen[0][0], seen
