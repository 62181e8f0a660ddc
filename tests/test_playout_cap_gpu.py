"""Playout cap randomization on the GPU ("playout_cap_sims" / "playout_cap_full_e6", include/az_engine.h), held to the project's bar:
bit-exact against the twin (tests/cpp/selfplay_twin.cpp -- the unchanged oracle with the feature restated around it, and the g++
build of the predicate the kernels compile) on every path a self-play move can take, and bit for bit WITHOUT effect where it must have
none.

Shapes: 100 episodes on 40 slots = one whole 256-lane tree workgroup (32 games) plus one partial wave, with slot refill.  (N, n) =
(24, 8) with one and four simulation threads; (44, 12), where a fast budget ends inside the first replayed 20-step graph chunk and a full
one after two chunks and a remainder; (25, 5) on Connect Three.  Every parity test asserts that between 10 % and 90 % of the plies it
compared were full moves and that both kinds occur at ply 0 (seeds 11 / 12, P = 0.25 / 0.5: tests/test_playout_cap_cpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import selfplay_twin as pc      # noqa: E402

HASH_SALT, MODEL_SALT = 1234, 0x51ED27
AZ_ERR_BAD_ARGUMENT = 1
N_GAMES, SLOTS = 100, 40
COUNTERS = ("simulations", "leaf_evals", "expansions", "link_hits", "terminal_hits", "moves", "samples", "games")


def oracle_salt(model_id):
    return HASH_SALT + model_id * MODEL_SALT


def _restore(e):
    e.selfplay_end()
    e.set_option("playout_cap_sims", 0)
    e.set_option("playout_cap_full_e6", 250000)
    e.set_root_noise(0.0, 1.0)
    for k, v in (("eval_dedup", 1), ("fused_search", 1), ("selfplay_async", 0)):
        e.set_option(k, v)


@pytest.fixture(autouse=True)
def cap_off_afterwards(engine):
    """The session's engine is shared with every other module: leave it as it was found."""
    yield
    _restore(engine)


@pytest.fixture(scope="module")
def engine3(engine_mod):
    """The seam's second game (AZ_GAME_CONNECT_THREE)."""
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128, game=engine_mod.GAME_CONNECT_THREE)
    e.net_set_kind(10, engine_mod.NET_HASH, HASH_SALT)
    yield e
    e.close()


def capped_selfplay(e, sims, cap_sims, full_e6, seed, threads=1, options=None, concurrent=SLOTS, n_games=N_GAMES, first_game_id=1000, model_id=10,
                    **kw):
    for k, v in (options or {}).items():
        e.set_option(k, v)
    e.set_option("playout_cap_full_e6", full_e6)
    e.set_option("playout_cap_sims", cap_sims)
    e.reset_stats()
    got = e.selfplay(n_games=n_games, num_sims=sims, model_id=model_id, seed=seed, first_game_id=first_game_id, concurrent=concurrent,
                     num_sim_threads=threads, **kw)
    got["full_masks"] = e.selfplay_full_plies()
    got["stats"] = e.stats()
    return got


def check_against_twin(got, ref, degenerate_ok=False):
    assert np.array_equal(got["game_len"], ref["game_len"])
    assert np.array_equal(got["moves"], ref["moves"])
    assert np.array_equal(got["full_masks"], ref["full_masks"])
    assert got["count"] == ref["count"] == 2 * pc.popcount(ref["full_masks"])
    assert np.array_equal(got["boards"].reshape(-1, 84), ref["boards"].reshape(-1, 84))
    assert np.array_equal(got["pis"].view(np.uint32), ref["pis"].view(np.uint32))
    assert np.array_equal(got["zs"].view(np.uint32), ref["zs"].view(np.uint32))
    full, plies = pc.popcount(ref["full_masks"]), int(ref["game_len"].sum())
    st = got["stats"]
    print("full plies %d of %d, simulations %d (twin %d), samples %d" % (full, plies, st["simulations"], ref["sims"], st["samples"]))
    assert st["simulations"] == ref["sims"] == ref["budgets"]
    assert st["samples"] == full and st["moves"] == plies
    if not degenerate_ok:
        assert 0.1 <= full / plies <= 0.9, (full, plies)
        first = sum(int(m) & 1 for m in ref["full_masks"])
        assert 0 < first < len(ref["full_masks"]), first


# ---- options ------------------------------------------------------------------------------------------------------------------------------
def test_option_ranges_and_open_session(engine, engine_mod):
    for key, bad in (("playout_cap_sims", (-1, 65536, 1 << 40)), ("playout_cap_full_e6", (-1, 1000001))):
        for v in bad:
            with pytest.raises(engine_mod.AzError) as ei:
                engine.set_option(key, v)
            assert ei.value.status == AZ_ERR_BAD_ARGUMENT, (key, v)
    for key, good in (("playout_cap_sims", (0, 1, 65535, 8)), ("playout_cap_full_e6", (0, 1, 1000000, 250000))):
        for v in good:
            engine.set_option(key, v)
    engine.set_option("playout_cap_sims", 0)
    engine.selfplay_begin(4, 10, 10, seed=1)
    try:
        for key, v in (("playout_cap_sims", 5), ("playout_cap_full_e6", 500000), ("playout_cap_sims", 0)):
            with pytest.raises(engine_mod.AzError) as ei:
                engine.set_option(key, v)
            assert ei.value.status == AZ_ERR_BAD_ARGUMENT
    finally:
        engine.selfplay_end()
    engine.set_option("playout_cap_sims", 5)            # accepted again once the session is closed


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
PER_SIM = {"fused_search": 0}
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
        _restore(engine3)


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
    full = [bin(int(m)).count("1") for m in one["full_masks"]]
    assert 0.1 <= sum(full) / int(one["game_len"].sum()) <= 0.9
    engine.selfplay_begin(N_GAMES, sims, 10, seed=seed, first_game_id=1000, concurrent=SLOTS)
    try:
        off = 0
        for lo, k in ((0, 30), (30, 30), (60, 40)):
            got = engine.selfplay_next(k)
            masks = engine.selfplay_full_plies()
            cnt = 2 * sum(full[lo:lo + k])
            assert got["count"] == cnt
            assert np.array_equal(masks, one["full_masks"][lo:lo + k])
            assert np.array_equal(got["game_len"], one["game_len"][lo:lo + k]) and np.array_equal(got["moves"], one["moves"][lo:lo + k])
            for key in ("states", "boards", "pis", "zs"):
                assert np.array_equal(got[key], one[key][off:off + cnt]), key
            off += cnt
        assert off == one["count"]
    finally:
        engine.selfplay_end()


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
            off = np.zeros(N_GAMES + 1, np.int64)
            off[1:] = np.cumsum(cnt)
            fs = np.concatenate([states[g, :cnt[g]] for g in range(N_GAMES)])
            fp = np.concatenate([pis[g, :cnt[g]] for g in range(N_GAMES)])
            fv = np.concatenate([vs[g, :cnt[g]] for g in range(N_GAMES)])
            ref = pc.selfplay(N_GAMES, sims, cap_sims=cap_sims, full_e6=full_e6, net_kind=pc.NET_REPLAY, seed=seed, first_game_id=1000, replay=(off, fs, fp, fv))
            assert not ref["replay_bad"].any()
            check_against_twin(got, ref)
            st = got["stats"]
            assert st["leaf_rows_requested"] == st["leaf_rows_executed"] + st["eval_cache_hits"] + st["eval_batch_dups"], st
    finally:
        e.close()


# ---- the arena and the tree calls never see it --------------------------------------------------------------------------------------------------------------
def _c4_play(mine, theirs, a):
    mask = mine | theirs
    nb = (mask + (1 << (a * 7))) & (0x3F << (a * 7))
    return theirs, mine | nb


def _other_entries(engine):
    out = list(engine.arena(16, 25, new_model_id=11, old_model_id=10, seed=4))
    out += list(engine.arena_get_moves(16))
    tb = engine.tree_create(6, reserve=pc.default_reserve(30), num_sims=30, max_depth=1000, model_id=10, cpuct=1)
    states = np.zeros((6, 2), np.uint64)
    for move in range(3):
        pi, counts, q = tb.get_action_prob(states, 1.0 if move < 2 else 0.0, seed=3, first_game_id=40)
        out += [pi, counts, q]
        states = np.array([_c4_play(int(s[0]), int(s[1]), int(np.argmax(c))) for s, c in zip(states, counts)], np.uint64)
    tb.close()
    shared = engine.tree_create(2, reserve=pc.default_reserve(30), num_sims=30, max_depth=1000, model_id=10, cpuct=1)
    shared.share(0)
    slot = shared.slot_acquire()
    s = (0, 0)
    for move in range(3):
        pi, counts, q = shared.slot_get_action_prob(slot, s, 1.0, seed=31, game_id=5)
        out += [pi, counts, q]
        s = _c4_play(s[0], s[1], int(np.argmax(counts)))
    shared.slot_release(slot)
    shared.close()
    return out


def test_arena_and_tree_calls_ignore_the_keys(engine):
    want = _other_entries(engine)
    capped_selfplay(engine, 24, 8, 250000, 11, n_games=16, concurrent=8)     # leaves a capped arena behind in the pool; the keys stay set
    got = _other_entries(engine)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ---- the two Coaches ------------------------------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_coach_agree_with_a_playout_cap(engine_mod, tmp_path):
    """tests/test_coach_gpu.py::test_python_and_cpp_coach_agree with Coach.playout_cap_sims / playout_cap_full set on both hosts:
    byte-identical files, written from the full moves only."""
    from alphazero_rs_amd.coach import Coach
    C, seed = 128, 11
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp")}
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=C)
    try:
        e.net_init_random(0, 3)
        e.set_option("train_epochs", 1)
        coach = Coach.setup(e, dirs["py"], 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 1, 32, 25, 1, 1000, 1, log=lambda m: None)
        coach.playout_cap_sims, coach.playout_cap_full = 5, 0.5
        orig = e.selfplay
        seen = []

        def spy(**kw):
            r = orig(**kw)
            seen.append((int(r["game_len"].sum()), r["count"], pc.popcount(e.selfplay_full_plies())))
            return r
        e.selfplay = spy
        rep = coach.learn(seed=seed)
        e.selfplay = orig
        e.selfplay(n_games=2, num_sims=25, model_id=0, seed=1)
        assert int(e.selfplay_full_plies()[0]) & 1 and e.stats()["samples"] > 0     # cleared behind the episodes: every ply is recorded again
    finally:
        e.close()
    assert len(seen) == 1 and seen[0][1] == seen[0][2] and 0.1 * seen[0][0] <= seen[0][1] <= 0.9 * seen[0][0], seen
    exe = os.path.join(tmp_path, "test_coach_options")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_options.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, dirs["cpp"], str(C), str(seed), "playout_cap_sims=5", "playout_cap_full=0.5"], check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    crep = json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    assert len(rep) == len(crep) == 1
    for k in ("iteration", "samples", "nwins", "pwins", "draws", "accepted", "model_id"):
        assert rep[0][k] == crep[0][k], k
    files = sorted(os.listdir(dirs["py"]))
    assert files == sorted(os.listdir(dirs["cpp"])) and "0.examples" in files and "1.aznet" in files
    for f in files:
        with open(os.path.join(dirs["py"], f), "rb") as x, open(os.path.join(dirs["cpp"], f), "rb") as y:
            assert x.read() == y.read(), f
