"""az_tournament on the GPU (include/az_engine.h): one batched round robin against the pairwise az_arena calls it
replaces, on the same engine -- code the tournament leaves alone.  Game g of pair p must be game g of that pair's arena bit for bit:
result, length, every move and the opening.  Shapes are the smallest that cross the new kernels' boundaries: a model's batch of 36 trees
is one whole 32-tree workgroup plus a partial one."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg       # noqa: E402

pytestmark = pytest.mark.gpu

SALTS = (97531, 24680, 13579)
HASH_IDS = (60, 61, 62)
CONV_IDS = (70, 71, 72)
STAT_KEYS = ("games", "moves", "simulations", "expansions", "leaf_evals", "link_hits", "terminal_hits", "depth_sum", "leaf_rows_requested")


def pairs_of(ids):
    return list(itertools.combinations(range(len(ids)), 2))


def pairwise(e, ids, n, sims, seed=0, **kw):
    """The reference: one az_arena per pair, in the pairs' order.  wld [K,K,3] and the games' records, concatenated."""
    K = len(ids)
    out = dict(wld=np.zeros((K, K, 3), np.uint64), results=[], game_len=[], moves=[], boards=[], open_len=[], open_moves=[])
    for i, j in pairs_of(ids):
        wld, res = e.arena(n, sims, new_model_id=ids[i], old_model_id=ids[j], seed=seed, **kw)
        out["wld"][i, j] = wld
        out["wld"][j, i] = (wld[1], wld[0], wld[2])
        glen, gmoves = e.arena_get_moves(n)
        b, ln, mv = e.arena_get_openings(n)
        for key, v in (("results", res), ("game_len", glen), ("moves", gmoves), ("boards", b), ("open_len", ln), ("open_moves", mv)):
            out[key].append(v.copy())
    return {k: (v if k == "wld" else np.concatenate(v)) for k, v in out.items()}


def tournament(e, ids, n, sims, seed=0, **kw):
    got = e.tournament(ids, n, sims, seed=seed, **kw)
    games = len(pairs_of(ids)) * n
    got["boards"], got["open_len"], got["open_moves"] = e.arena_get_openings(games)
    return got


def assert_same_games(got, ref):
    for key in ("wld", "results", "game_len", "moves", "boards", "open_len", "open_moves"):
        assert got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), key


@pytest.fixture
def hash_engine(engine):
    """The session engine with three hash models of different salts, openings off before and after."""
    for mid, salt in zip(HASH_IDS, SALTS):
        engine.net_set_kind(mid, 1, salt)
    engine.set_arena_openings(0)
    engine.arena_set_opening_book(None)
    yield engine
    engine.set_arena_openings(0)
    engine.arena_set_opening_book(None)


@pytest.fixture(scope="module")
def engine3(engine_mod):
    yield from fg.connect_three_engine(engine_mod)


def test_hash_nets_match_the_pairwise_arenas(hash_engine):
    """Three hash models, n = 18: 36 trees per model, 54 games.  Also the counters: the sums over the three arena calls."""
    e = hash_engine
    e.set_arena_openings(4)
    e.reset_stats()
    ref = pairwise(e, HASH_IDS, 18, 25, seed=5)
    st_ref = e.stats()
    e.reset_stats()
    got = tournament(e, HASH_IDS, 18, 25, seed=5)
    st = e.stats()
    assert_same_games(got, ref)
    assert len(got["results"]) == 54 and (got["open_len"] == 4).all()
    assert int(got["wld"].sum()) == 2 * 54 and not got["wld"][np.arange(3), np.arange(3)].any()
    # every pair of models plays the same n / 2 openings in both seatings
    b = got["boards"].reshape(3, 2, 9, 2)
    assert np.array_equal(b[:, 0], b[:, 1]) and np.array_equal(b[0], b[1]) and np.array_equal(b[0], b[2])
    assert len({tuple(x) for x in b[0, 0].tolist()}) > 1
    assert len({tuple(m) for m in got["moves"].tolist()}) > 6          # not one of two games per pair
    for k in STAT_KEYS:
        print(k, st[k], st_ref[k])
        assert st[k] == st_ref[k], k
    print("leaf_rows_executed", st["leaf_rows_executed"], st_ref["leaf_rows_executed"])
    assert st["leaf_rows_executed"] <= st_ref["leaf_rows_executed"]
    assert st["games"] == 54 and st["simulations"] == 25 * int(got["game_len"].sum())


def test_counters_with_leaf_batches(hash_engine):
    """The same sums where the searches go through leaf batches, election tables and the evaluation cache ("eval_dedup" 2 reaches the hash
    nets): requested rows add up, executed rows are no more than the pairwise calls'."""
    e = hash_engine
    e.set_arena_openings(4)
    e.set_option("eval_dedup", 2)
    try:
        e.reset_stats()
        ref = pairwise(e, HASH_IDS, 18, 25, seed=6)
        st_ref = e.stats()
        e.reset_stats()
        got = tournament(e, HASH_IDS, 18, 25, seed=6)
        st = e.stats()
    finally:
        e.set_option("eval_dedup", 1)
    assert_same_games(got, ref)
    for k in STAT_KEYS:
        print(k, st[k], st_ref[k])
        assert st[k] == st_ref[k], k
    print("leaf_rows_executed", st["leaf_rows_executed"], st_ref["leaf_rows_executed"])
    assert 0 < st["leaf_rows_executed"] <= st_ref["leaf_rows_executed"]


def test_two_simulations_in_flight(hash_engine):
    e = hash_engine
    e.set_arena_openings(4)
    ref = pairwise(e, HASH_IDS, 18, 26, seed=7, num_sim_threads=2)
    assert_same_games(tournament(e, HASH_IDS, 18, 26, seed=7, num_sim_threads=2), ref)


def test_opening_book(hash_engine):
    e = hash_engine
    book = np.array([fg.c4_play(0, 0, 3), fg.c4_play(*fg.c4_play(0, 0, 2), 4), fg.c4_play(*fg.c4_play(0, 0, 0), 6)], np.uint64)
    e.arena_set_opening_book(book)
    e.set_arena_openings(2)
    ref = pairwise(e, HASH_IDS, 18, 25, seed=8)
    got = tournament(e, HASH_IDS, 18, 25, seed=8)
    assert_same_games(got, ref)
    e.set_arena_openings(0)                                         # the book alone
    assert_same_games(tournament(e, HASH_IDS, 8, 25, seed=8), pairwise(e, HASH_IDS, 8, 25, seed=8))


def test_connect_three(engine3, engine_mod):
    e = engine3
    ids = (10, 21, 22)
    e.net_set_kind(21, engine_mod.NET_HASH, SALTS[1])
    e.net_set_kind(22, engine_mod.NET_HASH, SALTS[2])
    e.set_arena_openings(2)
    try:
        ref = pairwise(e, ids, 18, 25, seed=9)
        assert_same_games(tournament(e, ids, 18, 25, seed=9), ref)
    finally:
        e.set_arena_openings(0)


def test_two_models_are_one_arena(hash_engine):
    e = hash_engine
    e.set_arena_openings(4)
    ids = (HASH_IDS[2], HASH_IDS[0])
    wld, res = e.arena(18, 25, new_model_id=ids[0], old_model_id=ids[1], seed=11)
    glen, gmoves = e.arena_get_moves(18)
    got = tournament(e, ids, 18, 25, seed=11)
    assert np.array_equal(got["results"], res) and np.array_equal(got["game_len"], glen) and np.array_equal(got["moves"], gmoves)
    assert got["wld"][0, 1].tolist() == wld.tolist() and got["wld"][1, 0].tolist() == [wld[1], wld[0], wld[2]]


@pytest.fixture(scope="module")
def conv_engine(engine):
    """Three random-init conv models on the session engine; freed, with every option back, afterwards."""
    for k, mid in enumerate(CONV_IDS):
        engine.net_init_random(mid, seed=100 + k)
    yield engine
    engine.set_eval_mirror(False)
    engine.set_arena_openings(0)
    for mid in CONV_IDS:
        engine.net_free(mid)


@pytest.mark.parametrize("variant", ["plain", "one_fp8", "eval_mirror"])
def test_conv_nets_match_the_pairwise_arenas(conv_engine, engine_mod, variant):
    e = conv_engine
    e.set_arena_openings(2)
    if variant == "one_fp8":
        e.net_set_class(CONV_IDS[1], engine_mod.NET_CLASS_FP8)
    if variant == "eval_mirror":
        e.set_eval_mirror(True)
    try:
        e.reset_stats()
        ref = pairwise(e, CONV_IDS, 4, 16, seed=12)
        st_ref = e.stats()
        e.reset_stats()
        got = tournament(e, CONV_IDS, 4, 16, seed=12)
        st = e.stats()
    finally:
        e.net_set_class(CONV_IDS[1], engine_mod.NET_CLASS_ENGINE)
        e.set_eval_mirror(False)
        e.set_arena_openings(0)
    assert_same_games(got, ref)
    for k in STAT_KEYS:
        assert st[k] == st_ref[k], k
    print("leaf_rows_executed", st["leaf_rows_executed"], st_ref["leaf_rows_executed"])
    assert 0 < st["leaf_rows_executed"] <= st_ref["leaf_rows_executed"]


def test_purity(hash_engine):
    """The other entry points before and after a tournament; two tournaments in a row; the tree pool keeps what an arena leaves."""
    e = hash_engine
    before = fg.other_entry_points(e)
    e.set_arena_openings(4)
    a = tournament(e, HASH_IDS, 18, 25, seed=13)
    b = tournament(e, HASH_IDS, 18, 25, seed=13)
    allocs = e.stats()["tree_arena_allocs"]
    c = tournament(e, HASH_IDS, 18, 25, seed=13)
    e.set_arena_openings(0)
    assert_same_games(b, a)
    assert_same_games(c, a)
    assert e.stats()["tree_arena_allocs"] == allocs                # a third call of the same shape allocates no tree arena
    with pytest.raises(Exception):
        e.arena_get_evals(0, 54, 8)                                # there is no eval log here
    fg.assert_same_outputs(fg.other_entry_points(e), before)


def test_arena_tournament_arena_share_streams_and_trees(hash_engine):
    """az_arena with eval logs, az_tournament of three models, the same az_arena again: the order in which the two entry points reuse the
    engine's side streams, workspaces and leased tree arenas.  The two arenas agree in every output, eval logs included; the tournament in
    between leaves no eval log.  (One launch per simulation step: the path that writes the log rows.)"""
    e = hash_engine
    n, sims, cap = 16, 25, 21 * 26 + 8
    e.set_arena_openings(4)
    e.set_option("fused_search", 0)

    def arena():
        out = list(e.arena(n, sims, new_model_id=HASH_IDS[0], old_model_id=HASH_IDS[1], seed=15, record_evals=cap))
        out += list(e.arena_get_moves(n)) + list(e.arena_get_openings(n))
        for which in (0, 1):
            cnt, states, pis, vs = e.arena_get_evals(which, n, cap)
            assert 0 < cnt.min() and cnt.max() <= cap
            live = np.arange(cap)[None, :] < cnt[:, None]                # rows behind a game's count are never written
            out += [cnt, states[live], pis[live], vs[live]]
        return out
    try:
        first = arena()
        got = tournament(e, HASH_IDS, 18, sims, seed=13)
        with pytest.raises(Exception):
            e.arena_get_evals(0, 54, cap)
        second = arena()
    finally:
        e.set_option("fused_search", 1)
        e.set_arena_openings(0)
    assert len(got["results"]) == 54
    assert len(first) == len(second) == 15
    for a, b in zip(first, second):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_refusals(hash_engine, engine_mod):
    """Every refusal: AZ_ERR_BAD_ARGUMENT, the sentinel-filled outputs untouched, the previous move record still served."""
    e = hash_engine
    e.arena(16, 25, new_model_id=HASH_IDS[0], old_model_id=HASH_IDS[1], seed=3)
    record = e.arena_get_moves(16) + e.arena_get_openings(16)
    e.net_init_random(73, seed=1)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ok = dict(ids=list(HASH_IDS), n=4, sims=25, max_depth=1000, threads=1, reserve=1000000)
    cases = [("K = 1", dict(ids=[60])), ("K = 0", dict(ids=[])), ("K = 17", dict(ids=list(range(200, 217)))), ("odd n", dict(n=5)), ("n = 0", dict(n=0)),
             ("n < 0", dict(n=-2)), ("too many games", dict(n=21846)), ("no ids", dict(ids=None)), ("no wld", dict(wld=None)),
             ("repeated id", dict(ids=[60, 61, 60])), ("unknown id", dict(ids=[60, 61, 999])), ("conv batch", dict(ids=[60, 73], n=8194)),
             ("num_sims", dict(sims=0)), ("max_depth", dict(max_depth=-1)), ("reserve", dict(reserve=7)), ("threads", dict(threads=9)),
             ("sims % threads", dict(threads=2)), ("session", dict(session=True))]
    try:
        for name, change in cases:
            a = dict(ok, **change)
            ids = None if a["ids"] is None else np.array(a["ids"] + [0], np.int32)            # (never empty: a real pointer for K = 0)
            K = 3 if a["ids"] is None else len(a["ids"])
            wld = np.full((17, 17, 3), 77, np.uint64)
            res = np.full(70000, 77, np.int8)
            if a.get("session"):
                e.selfplay_begin(4, 10, 10, seed=1)
            try:
                st = e._lib.az_tournament(e._h, ptr(ids), K, a["n"], a["sims"], a["max_depth"], 1, a["threads"], a["reserve"], 5,
                                          None if "wld" in change else ptr(wld), ptr(res))
            finally:
                if a.get("session"):
                    e.selfplay_end()
            assert st == fg.AZ_ERR_BAD_ARGUMENT, name
            assert (wld == 77).all() and (res == 77).all(), name
            now = e.arena_get_moves(16) + e.arena_get_openings(16)
            assert all(np.array_equal(x, y) for x, y in zip(now, record)), name
    finally:
        e.net_free(73)


def test_move_quality_runs_on_the_records(hash_engine):
    e = hash_engine
    e.set_arena_openings(4)
    ref = pairwise(e, HASH_IDS, 18, 25, seed=14)
    want = e.move_quality(ref["game_len"], ref["moves"], ref["boards"], min_stones=26)
    got = tournament(e, HASH_IDS, 18, 25, seed=14)
    glen, gmoves = e.arena_get_moves(54)
    have = e.move_quality(glen, gmoves, got["boards"], min_stones=26)
    assert np.array_equal(have[0], want[0]) and np.array_equal(have[1], want[1])
    assert (want[0] != 0).any()


def test_cpp_host_matches_python(engine_mod, tmp_path):
    """tests/cpp/test_tournament.cpp: the hash-net case through az_host::tournament and az_host::rating_fit, exactly the Python host's."""
    exe = os.path.join(tmp_path, "test_tournament")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_tournament.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, "18", "25", "4", "5"] + [str(s) for s in SALTS], check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
    cpp = json.loads(out.strip().splitlines()[-1])
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    try:
        for mid, salt in zip(HASH_IDS, SALTS):
            e.net_set_kind(mid, engine_mod.NET_HASH, salt)
        e.set_arena_openings(4)
        got = e.tournament(HASH_IDS, 18, 25, seed=5)
    finally:
        e.close()
    elo, se, sweeps = engine_mod.rating_fit(got["wld"])
    assert cpp["wld"] == got["wld"].reshape(-1).tolist() and cpp["results"] == got["results"].tolist()
    assert cpp["game_len"] == got["game_len"].tolist() and cpp["moves"] == got["moves"].reshape(-1).tolist()
    assert cpp["sweeps"] == sweeps and cpp["elo"] == elo.tolist() and cpp["elo_se"] == se.tolist()
