"""What the GPU test modules of the opt-in features share (root noise, playout cap, forced playouts, mirror-canonical evaluation, paired
arena openings): the constants, the helpers that drive the engine, and the comparators that hold its output to the twin
(tests/selfplay_twin.py), to a one-call run and to the other host.  TEST INFRASTRUCTURE ONLY.  A plain module, imported the way
selfplay_twin is; the modules keep their shape tables, their feature conditions and the tests that have no twin elsewhere.
tests/test_feature_gpu_harness_cpu.py checks without a GPU that every comparator here fails on each field it claims to compare."""
import json
import os
import subprocess

import numpy as np
import pytest

import selfplay_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH_SALT, MODEL_SALT = 1234, 0x51ED27
AZ_ERR_BAD_ARGUMENT = 1
N_GAMES, SLOTS = 100, 40      # one whole 256-lane tree workgroup (32 games) plus one partial wave, with slot refill
COUNTERS = ("simulations", "leaf_evals", "expansions", "link_hits", "terminal_hits", "moves", "samples", "games")
PER_SIM = {"fused_search": 0}
REPORT_KEYS = ("iteration", "samples", "nwins", "pwins", "draws", "accepted", "model_id")


def oracle_salt(model_id):
    return HASH_SALT + model_id * MODEL_SALT


def restore(e):
    """Every self-play option a feature module touches back at the engine's default."""
    e.selfplay_end()
    e.set_forced_playouts(0.0, False)
    e.set_option("playout_cap_sims", 0)
    e.set_option("playout_cap_full_e6", 250000)
    e.set_root_noise(0.0, 1.0)
    for k, v in (("eval_dedup", 1), ("fused_search", 1), ("selfplay_async", 0)):
        e.set_option(k, v)


def connect_three_engine(engine_mod):
    """The body of the modules' engine3 fixture: an engine of the seam's second game (AZ_GAME_CONNECT_THREE) with the hash net as model 10."""
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128, game=engine_mod.GAME_CONNECT_THREE)
    e.net_set_kind(10, engine_mod.NET_HASH, HASH_SALT)
    yield e
    e.close()


def c4_play(mine, theirs, a):
    mask = mine | theirs
    nb = (mask + (1 << (a * 7))) & (0x3F << (a * 7))
    return theirs, mine | nb


# ---- self-play under the options ----------------------------------------------------------------------------------------------------------
def run_selfplay(e, sims, seed, *, cap=None, forced=None, noise=None, threads=1, options=None, concurrent=SLOTS, n_games=N_GAMES,
                 first_game_id=1000, model_id=10, **kw):
    """One az_selfplay with cap = (cap_sims, full_e6), noise = (eps, alpha) and forced = (k, prune) set first, in this order behind the
    plain options; a feature that is not named is not touched.  The engine's dict plus full_masks and stats (reset before the call)."""
    for k, v in (options or {}).items():
        e.set_option(k, v)
    if cap is not None:
        e.set_option("playout_cap_full_e6", cap[1])
        e.set_option("playout_cap_sims", cap[0])
    if noise is not None:
        e.set_root_noise(*noise)
    if forced is not None:
        e.set_forced_playouts(*forced)
    e.reset_stats()
    got = e.selfplay(n_games=n_games, num_sims=sims, model_id=model_id, seed=seed, first_game_id=first_game_id, concurrent=concurrent,
                     num_sim_threads=threads, **kw)
    got["full_masks"] = e.selfplay_full_plies()
    got["stats"] = e.stats()
    return got


def same_rows(a, b):
    """Two arrays of one dtype hold the same rows, as bytes (the trailing shape may differ: boards [n,2,6,7] or [n,84])."""
    flat = lambda x: np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    return a.dtype == b.dtype and len(a) == len(b) and np.array_equal(flat(a), flat(b))


def check_tuples_against_twin(got, ref, step=1):
    """game_len, moves and the (board, pi, z) tuples, bit for bit.  step 2: `got` was played without symmetries and holds every second
    tuple of the twin's, which always emits a tuple and its mirror image."""
    assert np.array_equal(got["game_len"], ref["game_len"])
    assert np.array_equal(got["moves"], ref["moves"])
    assert got["count"] * step == ref["count"]
    for key in ("boards", "pis", "zs"):
        assert same_rows(got[key], ref[key][::step]), key


def check_samples_against_twin(got, ref):
    """A run_selfplay result against the twin's: the tuples, the full-move masks and the engine's counters.  Returns (full moves, plies)."""
    check_tuples_against_twin(got, ref)
    assert np.array_equal(got["full_masks"], ref["full_masks"])
    full, plies = tw.popcount(ref["full_masks"]), int(ref["game_len"].sum())
    assert got["count"] == ref["count"] == 2 * full
    st = got["stats"]
    print("full plies %d of %d, simulations %d (twin %d), samples %d" % (full, plies, st["simulations"], ref["sims"], st["samples"]))
    assert st["simulations"] == ref["sims"] == ref["budgets"]
    assert st["samples"] == full and st["moves"] == plies and st["games"] == len(ref["game_len"])
    return full, plies


def check_session_in_chunks(engine, one, chunks, begin_kwargs):
    """selfplay_begin(**begin_kwargs), one selfplay_next(k) per (lo, k) of `chunks`, selfplay_end: every chunk is the slice of `one` --
    a one-call run of the same episodes, or the twin's -- in tuples, game_len, moves and full-move masks."""
    full = [tw.popcount(m) for m in one["full_masks"]]
    engine.selfplay_begin(**begin_kwargs)
    try:
        off = 0
        for lo, k in chunks:
            got = engine.selfplay_next(k)
            masks = engine.selfplay_full_plies()
            cnt = 2 * sum(full[lo:lo + k])
            assert got["count"] == cnt
            assert np.array_equal(masks, one["full_masks"][lo:lo + k])
            assert np.array_equal(got["game_len"], one["game_len"][lo:lo + k]) and np.array_equal(got["moves"], one["moves"][lo:lo + k])
            for key in ("states", "boards", "pis", "zs"):
                if key in one:                                  # the twin has no packed states
                    assert same_rows(got[key], one[key][off:off + cnt]), key
            off += cnt
        assert off == one["count"]
    finally:
        engine.selfplay_end()


def flatten_eval_log(cnt, states, pis, vs):
    """A per-game eval log ([n] counts, [n, cap, ...] rows) as the twin's ReplayNet reads it: offsets [n + 1] and the rows back to back."""
    n = len(cnt)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(cnt)
    fs, fp, fv = (np.concatenate([a[g, :cnt[g]] for g in range(n)]) for a in (states, pis, vs))
    return off, fs, fp, fv


# ---- options ------------------------------------------------------------------------------------------------------------------------------
def check_option_ranges(engine, engine_mod, bad, good, locked, settle, reopen):
    """bad / good: ((key, values), ...) refused with AZ_ERR_BAD_ARGUMENT / accepted; settle() leaves a legal state behind them; locked:
    ((key, value), ...) refused while a session is open; reopen: a (key, value) accepted again once it is closed."""
    for key, values in bad:
        for v in values:
            with pytest.raises(engine_mod.AzError) as ei:
                engine.set_option(key, v)
            assert ei.value.status == AZ_ERR_BAD_ARGUMENT, (key, v)
    for key, values in good:
        for v in values:
            engine.set_option(key, v)
    settle()
    engine.selfplay_begin(4, 10, 10, seed=1)
    try:
        for key, v in locked:
            with pytest.raises(engine_mod.AzError) as ei:
                engine.set_option(key, v)
            assert ei.value.status == AZ_ERR_BAD_ARGUMENT, (key, v)
    finally:
        engine.selfplay_end()
    engine.set_option(*reopen)


# ---- the entry points a self-play option must not reach -----------------------------------------------------------------------------------
def arena_outputs(engine):
    return list(engine.arena(16, 25, new_model_id=11, old_model_id=10, seed=4)) + list(engine.arena_get_moves(16))


def other_entry_points(engine):
    """An arena, three moves of a six-tree batch and three of one slot of a shared batch: every output, in order."""
    out = arena_outputs(engine)
    tb = engine.tree_create(6, reserve=tw.default_reserve(30), num_sims=30, max_depth=1000, model_id=10, cpuct=1)
    states = np.zeros((6, 2), np.uint64)
    for move in range(3):
        pi, counts, q = tb.get_action_prob(states, 1.0 if move < 2 else 0.0, seed=3, first_game_id=40)
        out += [pi, counts, q]
        states = np.array([c4_play(int(s[0]), int(s[1]), int(np.argmax(c))) for s, c in zip(states, counts)], np.uint64)
    tb.close()
    shared = engine.tree_create(2, reserve=tw.default_reserve(30), num_sims=30, max_depth=1000, model_id=10, cpuct=1)
    shared.share(0)
    slot = shared.slot_acquire()
    s = (0, 0)
    for move in range(3):
        pi, counts, q = shared.slot_get_action_prob(slot, s, 1.0, seed=31, game_id=5)
        out += [pi, counts, q]
        s = c4_play(s[0], s[1], int(np.argmax(counts)))
    shared.slot_release(slot)
    shared.close()
    return out


def assert_same_outputs(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ---- the two Coaches ----------------------------------------------------------------------------------------------------------------------
def compare_directories(a, b, required=("0.examples", "1.aznet")):
    """Two checkpoint directories hold the same files, the `required` ones among them, byte for byte.  Returns the sorted names."""
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)), (files, sorted(os.listdir(b)))
    for f in required:
        assert f in files, f
    for f in files:
        with open(os.path.join(a, f), "rb") as x, open(os.path.join(b, f), "rb") as y:
            assert x.read() == y.read(), f
    return files


def run_coach_pair(engine_mod, tmp_path, cpp_args, configure, *, num_eps=32, inspect=None, plain=None):
    """tests/test_coach_gpu.py::test_python_and_cpp_coach_agree in miniature (one iteration, C = 128, seed 11) with a feature set on both
    hosts: configure(coach, engine) on the Python Coach before learn(), `cpp_args` ("key=value") for tests/cpp/test_coach_options.cpp.
    Same report, byte-identical files.  inspect(engine) sees the Python run's engine behind learn(), still open.  plain(coach, engine)
    configures a control run with the feature off, whose 0.examples must differ."""
    from alphazero_rs_amd.coach import Coach
    C, seed = 128, 11
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp", "plain")}

    def run_py(d, configure, inspect=None):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=C)
        try:
            e.net_init_random(0, 3)
            e.set_option("train_epochs", 1)
            coach = Coach.setup(e, d, 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 1, num_eps, 25, 1, 1000, 1, log=lambda m: None)
            configure(coach, e)
            rep = coach.learn(seed=seed)
            if inspect is not None:
                inspect(e)
            return rep
        finally:
            e.close()
    rep = run_py(dirs["py"], configure, inspect)
    if plain is not None:
        run_py(dirs["plain"], plain)
    exe = os.path.join(tmp_path, "test_coach_options")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_options.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, dirs["cpp"], str(C), str(seed), *cpp_args], check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    crep = json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    assert len(rep) == len(crep) == 1
    for k in REPORT_KEYS:
        assert rep[0][k] == crep[0][k], k
    compare_directories(dirs["py"], dirs["cpp"])
    if plain is not None:
        with open(os.path.join(dirs["py"], "0.examples"), "rb") as x, open(os.path.join(dirs["plain"], "0.examples"), "rb") as y:
            assert x.read() != y.read()
