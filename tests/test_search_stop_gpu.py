"""The decided-move stop on the GPU (include/az_search_stop.h, csrc/az_stop.h), held to the project's bar: an eligible
search returns the full search's move and pi and, in everything else, the feature-off search of as many simulations as it ran -- bit for
bit, on both search kernels; self-play and the arena match the twin (tests/cpp/stop_twin.cpp: the unchanged oracle with the rule restated
around it) tuple for tuple and move for move; and where no move is eligible nothing changes at all.

Shapes: 40 trees / 100 episodes on 40 slots / 40 arena games = one whole 256-lane tree workgroup (32 trees) plus one partial wave.
B = 32 crosses one replayed 20-step graph chunk plus a remainder of launches; B = 16 on the conv engine stays below a chunk."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg            # noqa: E402
import search_stop_roots as roots   # noqa: E402
import stop_twin as st              # noqa: E402
from feature_gpu import AZ_ERR_BAD_ARGUMENT, HASH_SALT, N_GAMES, SLOTS, oracle_salt      # noqa: E402

B = 32
STATES = np.array(roots.ROOTS, np.uint64)
RESERVE = st.default_reserve(64)


@pytest.fixture(autouse=True)
def stop_off_afterwards(engine):
    """The session's engine is shared with every other module: leave it as it was found."""
    yield
    engine.selfplay_end()
    engine.set_search_stop(0)
    engine.set_arena_openings(0)
    engine.set_gumbel(0)
    fg.restore(engine)
    engine.search_stop_stats(reset=True)


@pytest.fixture(scope="module")
def conv_engine(engine_mod):
    """A random-init conv net at 128 channels as model 0, and the same weights pinned to the fp8 class as model 1."""
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    e.net_init_random(0, 3)
    e.net_init_random(1, 3)
    e.net_set_class(1, engine_mod.NET_CLASS_FP8)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def tree_call(e, model_id, sims, on, temp=0.0):
    """One az_tree_get_action_prob of a fresh 40-tree batch built at the roots; on = None leaves the switch as it stands."""
    tb = e.tree_create(len(STATES), reserve=RESERVE, num_sims=sims, max_depth=1000, model_id=model_id, cpuct=1)
    try:
        tb.reset(STATES)
        if on is not None:
            e.set_search_stop(1 if on else 0)
        return tb.get_action_prob(STATES, temp, seed=5, first_game_id=9)
    finally:
        if on is not None:
            e.set_search_stop(0)
        tb.close()


_OFF = {}


def off_runs(e, key, model_id, budget):
    """The feature-off runs at num_sims = 1 .. budget (az_tree_create refuses 0, and a fresh root, all counts 0, is never decided before its
    first simulation), computed once per configuration and shared."""
    if key not in _OFF:
        _OFF[key] = {k: tree_call(e, model_id, k, False) for k in range(1, budget + 1)}
    return _OFF[key]


def check_prefix(e, key, model_id, budget, min_stopped, twin=None):
    off = off_runs(e, key, model_id, budget)
    e.reset_stats()
    e.search_stop_stats(reset=True)
    pi, counts, q = tree_call(e, model_id, budget, True)
    sims, ctr = e.stats()["simulations"], e.search_stop_stats(reset=True)
    ran = counts.astype(np.int64).sum(axis=1)                    # a fresh root: i* = sum(counts)
    # the input condition, from the feature-off runs alone: the first i at which the rule holds on the off run's counts
    first = []
    for g in range(len(STATES)):
        hit = [i for i in range(1, budget) if st.decided_py(off[i][1][g], budget - i)]
        first.append(hit[0] if hit else budget)
    print("%s: stopped %d of %d trees, simulations run %s" % (key, sum(f < budget for f in first), len(first), first))
    assert sum(f < budget for f in first) >= min_stopped
    if twin is not None:
        assert sum(x < budget for x in twin) >= min_stopped and list(twin) == first
    for g in range(len(STATES)):
        i = int(ran[g])
        assert i == first[g], (g, i, first[g])                  # the rule holds at i* and fails at every smaller i
        assert np.array_equal(counts[g], off[i][1][g]) and np.array_equal(bits(q[g]), bits(off[i][2][g])), g      # prefix
        assert np.array_equal(bits(pi[g]), bits(off[budget][0][g])), g                                             # same move and pi
        assert pi[g].max() == 1.0 and pi[g].sum() == 1.0
    skipped = int(sum(budget - f for f in first))
    assert ctr == {"eligible_moves": len(STATES), "stopped_moves": sum(f < budget for f in first), "budgeted_sims": budget * len(STATES),
                   "skipped_sims": skipped}
    assert sims == budget * len(STATES) - skipped


# ---- 1. prefix and same move, on fresh roots --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,fused", [("hash", 1), ("hash", 0), ("stub", 1), ("stub", 0)])
def test_prefix_and_same_move_fixture_nets(engine, net, fused):
    """fused_search 1 runs k_search_fixture, 0 k_backup_select (launches and one replayed graph chunk)."""
    engine.set_option("fused_search", fused)
    model, kind, salt = (10, st.NET_HASH, oracle_salt(10)) if net == "hash" else (0, st.NET_STUB, 0)
    check_prefix(engine, net, model, B, 20, twin=roots.twin_runs(kind, salt, B))


@pytest.mark.parametrize("fused", [1, 0])
def test_prefix_and_same_move_with_root_noise(engine, fused):
    """Root noise only changes priors: the rule and both properties hold as they are (on and off runs draw the same noise)."""
    engine.set_option("fused_search", fused)
    engine.set_root_noise(0.25, 1.0)
    check_prefix(engine, "hash-noise", 10, B, 4)


@pytest.mark.parametrize("case", ["bf16", "mirror", "fp8"])
def test_prefix_and_same_move_conv(conv_engine, case):
    """B = 16 on the random-init conv net; with eval_mirror on; on the fp8-class model."""
    e = conv_engine
    e.set_eval_mirror(case == "mirror")
    try:
        check_prefix(e, "conv-" + case, 1 if case == "fp8" else 0, 16, 4)
    finally:
        e.set_eval_mirror(False)
        e.set_search_stop(0)


# ---- 2. a root decided before its first simulation; the graph key and the disarming ----------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_root_decided_before_its_first_simulation(engine, fused):
    """Two calls with the feature off (a lead can exceed 32 only after more than 32 visits), one with it on, one with it off again, all on the
    same az_tree: every call equals the twin's (stub net), trees whose lead already exceeds 32 return the second call's counts unchanged, and
    the fourth call -- the feature-off instantiation and graph again -- continues from the tree the stopped call left."""
    engine.set_option("fused_search", fused)
    tb = engine.tree_create(len(STATES), reserve=RESERVE, num_sims=B, max_depth=1000, model_id=0, cpuct=1)
    twins = [st.Tree(B, net_kind=st.NET_STUB, root=r, reserve=RESERVE) for r in roots.ROOTS]
    try:
        tb.reset(STATES)
        unchanged = 0
        prev = None
        for call, on in enumerate((0, 0, 1, 0)):
            engine.set_search_stop(on)
            engine.search_stop_stats(reset=True)
            pi, counts, q = tb.get_action_prob(STATES, 0.0, seed=5, first_game_id=9)
            ctr = engine.search_stop_stats(reset=True)
            want = [t.get_action_prob(r[0], r[1], 0.0, seed=5, game_id=9 + g, on=bool(on)) for g, (t, r) in enumerate(zip(twins, roots.ROOTS))]
            for g, (wpi, wcounts, wq, ran) in enumerate(want):
                assert np.array_equal(counts[g], wcounts) and np.array_equal(bits(q[g]), bits(wq)) and np.array_equal(bits(pi[g]), bits(wpi)), (call, g)
                if on and ran == 0:
                    assert np.array_equal(counts[g], prev[g])
                    unchanged += 1
            if on:
                assert ctr["eligible_moves"] == len(STATES) and ctr["skipped_sims"] == sum(B - w[3] for w in want)
                assert ctr["stopped_moves"] == sum(w[3] < B for w in want)
            else:
                assert ctr == dict.fromkeys(st.COUNTERS, 0)
            prev = counts
        assert unchanged >= 2, unchanged            # the one-move root and the immediate win at least
    finally:
        tb.close()
        for t in twins:
            t.close()


# ---- 3. self-play against the twin, tuple for tuple ---------------------------------------------------------------------------------------------
SP = dict(sims=B, seed=11, temp_threshold=4)
_TWIN = {}


def twin_selfplay(cap_sims=0):
    if cap_sims not in _TWIN:
        ref = st.selfplay(N_GAMES, SP["sims"], net_kind=st.NET_HASH, salt=oracle_salt(10), seed=SP["seed"], first_game_id=1000,
                          temp_threshold=SP["temp_threshold"], cap_sims=cap_sims, full_e6=500000)
        c = ref["ctr"]
        print("twin (cap %d): %s" % (cap_sims, c))
        # the input condition: the twin alone stops at least half of the eligible moves and skips at least 15 % of their budget
        assert 2 * c["stopped_moves"] >= c["eligible_moves"] > 0 and 100 * c["skipped_sims"] >= 15 * c["budgeted_sims"]
        _TWIN[cap_sims] = ref
    return _TWIN[cap_sims]


def check_eligible_one_hot(got, temp_threshold, full_masks):
    row = 0
    for g, n in enumerate(got["game_len"]):
        for ply in range(int(n)):
            if not (int(full_masks[g]) >> ply) & 1:
                continue
            for _ in range(2):
                if ply + 1 >= temp_threshold:
                    assert got["pis"][row].max() == 1.0 and got["pis"][row].sum() == 1.0, (g, ply)
                row += 1
    assert row == got["count"]


@pytest.mark.parametrize("fused,cap", [(1, 0), (0, 0), (1, 8), (0, 8)])
def test_selfplay_against_the_twin(engine, fused, cap):
    ref = twin_selfplay(cap)
    engine.set_search_stop(1)
    engine.search_stop_stats(reset=True)
    got = fg.run_selfplay(engine, SP["sims"], SP["seed"], temp_threshold=SP["temp_threshold"], options={"fused_search": fused},
                          cap=(cap, 500000) if cap else None)
    fg.check_tuples_against_twin(got, ref)
    assert np.array_equal(got["full_masks"], ref["full_masks"])
    assert engine.search_stop_stats() == ref["ctr"]
    assert got["stats"]["simulations"] == ref["sims"]
    check_eligible_one_hot(got, SP["temp_threshold"], ref["full_masks"])


def test_selfplay_session_in_two_chunks(engine):
    ref = twin_selfplay(0)
    engine.set_option("fused_search", 0)
    engine.set_search_stop(1)
    engine.search_stop_stats(reset=True)
    engine.reset_stats()
    fg.check_session_in_chunks(engine, ref, [(0, 60), (60, 40)],
                               dict(n_games=N_GAMES, num_sims=SP["sims"], model_id=10, seed=SP["seed"], first_game_id=1000, concurrent=SLOTS,
                                    temp_threshold=SP["temp_threshold"]))
    # the two chunks together played every episode to its end: the counters are the one call's
    assert engine.search_stop_stats() == ref["ctr"] and engine.stats()["simulations"] == ref["sims"]


# ---- 4. arena and tournament -----------------------------------------------------------------------------------------------------------------------
def test_arena_against_the_twin(engine):
    engine.set_arena_openings(4)
    out = {}
    for on in (0, 1):
        engine.set_search_stop(on)
        engine.reset_stats()
        engine.search_stop_stats(reset=True)
        wld, res = engine.arena(40, B, new_model_id=11, old_model_id=10, seed=4)
        ln, moves = engine.arena_get_moves(40)
        start = engine.arena_get_openings(40)[0]
        out[on] = (res, ln, moves, engine.stats(), engine.search_stop_stats(reset=True))
        tres, tmoves, tlen, tsims, tctr = st.arena(40, B, net_kind=st.NET_HASH, salt=HASH_SALT, seed=4, new_model_id=11, old_model_id=10, start=start,
                                                   on=bool(on))
        assert np.array_equal(res, tres) and np.array_equal(ln, tlen) and np.array_equal(moves, tmoves), on
        assert out[on][3]["simulations"] == tsims
        assert out[on][4] == (tctr if on else dict.fromkeys(st.COUNTERS, 0))
    ctr = out[1][4]
    print("arena: %s" % ctr)
    assert 2 * ctr["stopped_moves"] >= ctr["eligible_moves"] > 0
    assert out[1][3]["leaf_rows_requested"] < out[0][3]["leaf_rows_requested"]


def test_tournament_matches_its_arenas(engine):
    """Three models: game for game the three az_arena calls, with the feature on; fewer leaf rows than with it off."""
    ids, n = [0, 10, 11], 14
    engine.set_arena_openings(4)
    rows = {}
    for on in (0, 1):
        engine.set_search_stop(on)
        engine.reset_stats()
        t = engine.tournament(ids, n, B, seed=6)
        rows[on] = engine.stats()["leaf_rows_requested"]
    assert rows[1] < rows[0]
    tctr = engine.search_stop_stats(reset=True)
    p = 0
    total = dict.fromkeys(st.COUNTERS, 0)
    for i in range(3):
        for j in range(i + 1, 3):
            wld, res = engine.arena(n, B, new_model_id=ids[i], old_model_id=ids[j], seed=6)
            ln, moves = engine.arena_get_moves(n)
            assert np.array_equal(res, t["results"][p * n:(p + 1) * n]) and np.array_equal(ln, t["game_len"][p * n:(p + 1) * n])
            assert np.array_equal(moves, t["moves"][p * n:(p + 1) * n])
            for k, v in engine.search_stop_stats(reset=True).items():
                total[k] += v
            p += 1
    assert total == tctr and tctr["stopped_moves"] > 0


# ---- 5. reanalyse ---------------------------------------------------------------------------------------------------------------------------------
def test_reanalyse_rows_are_the_one_tree_calls(engine):
    engine.set_option("fused_search", 0)
    engine.set_search_stop(1)
    n = 12
    engine.search_stop_stats(reset=True)
    got = engine.reanalyse(B, 10, states=STATES[:n], temp=0.0, seed=5, first_game_id=9, concurrent=8, reserve=RESERVE)
    ctr = engine.search_stop_stats(reset=True)
    assert ctr["eligible_moves"] == n and ctr["stopped_moves"] >= 4
    skipped = 0
    for i in range(n):
        tb = engine.tree_create(1, reserve=RESERVE, num_sims=B, max_depth=1000, model_id=10, cpuct=1)
        tb.reset(STATES[i:i + 1])
        pi, counts, q = tb.get_action_prob(STATES[i:i + 1], 0.0, seed=5, first_game_id=9 + i)
        tb.close()
        assert np.array_equal(bits(got["pi"][i]), bits(pi[0])) and np.array_equal(got["counts"][i], counts[0]) and np.array_equal(bits(got["q"][i]), bits(q[0])), i
        skipped += B - int(counts[0].sum())
    assert engine.search_stop_stats(reset=True)["skipped_sims"] == skipped == ctr["skipped_sims"]


# ---- 6. ineligible moves --------------------------------------------------------------------------------------------------------------------------
def _ineligible_outputs(e):
    out = list(tree_call(e, 10, B, None, temp=1.0))
    for fused in (1, 0):
        got = fg.run_selfplay(e, 16, 3, temp_threshold=1000, options={"fused_search": fused}, n_games=48)
        out += [got[k] for k in ("game_len", "moves", "boards", "pis", "zs")] + [np.array([got["stats"]["simulations"]])]
    shared = e.tree_create(2, reserve=RESERVE, num_sims=B, max_depth=1000, model_id=10, cpuct=1)
    shared.share(0)
    slot = shared.slot_acquire()
    for r in roots.ROOTS[:3]:
        out += list(shared.slot_get_action_prob(slot, r, 0.0, seed=31, game_id=5))
    shared.slot_release(slot)
    shared.close()
    return out


def test_ineligible_moves_are_feature_off_output(engine):
    """A tree call at temp 1, self-play that never reaches temperature 0 and the slot calls: bit for bit the feature-off output, all four
    counters 0."""
    want = _ineligible_outputs(engine)
    engine.set_search_stop(1)
    engine.search_stop_stats(reset=True)
    got = _ineligible_outputs(engine)
    assert engine.get_search_stop() == 1 and len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), i
    assert engine.search_stop_stats() == dict.fromkeys(st.COUNTERS, 0)


# ---- 7. refusals and the session rule ---------------------------------------------------------------------------------------------------------------
def _refused(engine_mod, fn, *names):
    with pytest.raises(engine_mod.AzError) as ei:
        fn()
    assert ei.value.status == AZ_ERR_BAD_ARGUMENT, str(ei.value)
    for n in names:
        assert n in str(ei.value), str(ei.value)


def test_refusals_name_both_sides(engine, engine_mod):
    e = engine
    with pytest.raises(engine_mod.AzError) as ei:
        e.set_search_stop(2)
    assert ei.value.status == AZ_ERR_BAD_ARGUMENT and e.get_search_stop() == 0
    e.set_search_stop(1)
    assert e.get_search_stop() == 1
    snap = lambda: ({k: e.stats()[k] for k in fg.COUNTERS + ("leaf_rows_requested", "tree_launches")}, e.search_stop_stats())
    before = snap()
    tb1 = e.tree_create(4, reserve=RESERVE, num_sims=B, max_depth=1000, model_id=10, cpuct=1)
    tb2 = e.tree_create(4, reserve=RESERVE, num_sims=B, max_depth=1000, model_id=10, cpuct=1, num_threads=2)
    s4 = STATES[:4]
    entries = {
        "az_selfplay": lambda T: e.selfplay(n_games=4, num_sims=B, model_id=10, seed=1, num_sim_threads=T),
        "az_selfplay_begin": lambda T: e.selfplay_begin(4, B, 10, seed=1, num_sim_threads=T),
        "az_tree_get_action_prob": lambda T: (tb2 if T == 2 else tb1).get_action_prob(s4, 0.0),
        "az_reanalyse": lambda T: e.reanalyse(B, 10, states=s4, temp=0.0, num_sim_threads=T),
    }
    try:
        for name, call in entries.items():
            who = "az_selfplay" if name == "az_selfplay_begin" else name
            _refused(engine_mod, lambda: call(2), who, "search_stop", "num_sim_threads")
            e.set_option("selfplay_async", 1)
            _refused(engine_mod, lambda: call(1), who, "search_stop", "selfplay_async")
            e.set_option("selfplay_async", 0)
            e.set_gumbel(4)
            _refused(engine_mod, lambda: call(1), who, "search_stop", "gumbel_m")
            e.set_gumbel(0)
            e.set_forced_playouts(2.0, False)
            _refused(engine_mod, lambda: call(1), who, "search_stop", "forced_playouts_k_e6")
            e.set_forced_playouts(0.0, False)
        _refused(engine_mod, lambda: e.arena(4, B, 11, 10, num_sim_threads=2), "az_arena", "search_stop", "num_sim_threads")
        _refused(engine_mod, lambda: e.tournament([0, 10, 11], 2, B, num_sim_threads=2), "az_tournament", "search_stop", "num_sim_threads")
        assert snap() == before and e.get_search_stop() == 1
        # the arena and the tournament ignore the root rules and the free-running driver: they play
        e.set_forced_playouts(2.0, False)
        e.set_option("selfplay_async", 1)
        e.arena(4, B, 11, 10, seed=2)
    finally:
        tb1.close()
        tb2.close()


def test_setter_is_refused_beside_an_open_session(engine, engine_mod):
    """The session captured the switch at begin: the setter is refused, the stats entry is inert, the remaining chunks are the undisturbed ones."""
    ref = twin_selfplay(0)
    engine.set_option("fused_search", 0)
    engine.set_search_stop(1)
    engine.search_stop_stats(reset=True)
    engine.selfplay_begin(n_games=N_GAMES, num_sims=SP["sims"], model_id=10, seed=SP["seed"], first_game_id=1000, concurrent=SLOTS,
                          temp_threshold=SP["temp_threshold"])
    try:
        off = 0
        for lo, k in ((0, 60), (60, 40)):
            for v in (0, 1):
                _refused(engine_mod, lambda: engine.set_search_stop(v), "az_search_stop_set", "session")
            assert engine.get_search_stop() == 1
            mid = engine.search_stop_stats()
            assert mid == engine.search_stop_stats()
            got = engine.selfplay_next(k)
            cnt = got["count"]
            assert np.array_equal(got["game_len"], ref["game_len"][lo:lo + k]) and np.array_equal(got["moves"], ref["moves"][lo:lo + k])
            assert fg.same_rows(got["pis"], ref["pis"][off:off + cnt]) and fg.same_rows(got["zs"], ref["zs"][off:off + cnt])
            off += cnt
        assert off == ref["count"] and engine.search_stop_stats() == ref["ctr"]
    finally:
        engine.selfplay_end()
    engine.set_search_stop(0)


# ---- 8. the two Coaches ---------------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_coach_agree(engine_mod, tmp_path):
    """One iteration at 64 episodes and 16 simulations (C = 128, seed 11).  search_stop on: both hosts write identical files and count the same
    moves, and moves were stopped; off: both hosts' files equal those of a run that never touched the switch."""
    import json
    import subprocess
    from alphazero_rs_amd.coach import Coach
    C, seed, eps, sims = 128, 11, 64, 16
    tmp_path = str(tmp_path)

    def run_py(d, stop):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=C)
        try:
            e.net_init_random(0, 3)
            e.set_option("train_epochs", 1)
            coach = Coach.setup(e, d, 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 1, eps, sims, 1, 1000, 1, log=lambda m: None)
            if stop is not None:
                coach.search_stop = stop
            return coach.learn(seed=seed), e.search_stop_stats()
        finally:
            e.close()

    exe = os.path.join(tmp_path, "test_coach_search_stop")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_search_stop.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])

    def run_cpp(d, stop):
        out = subprocess.run([exe, d, str(C), str(seed), str(stop), str(eps), str(sims)], check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
        lines = out.strip().splitlines()
        return json.loads([l for l in lines if l.startswith("[")][-1]), json.loads([l for l in lines if l.startswith("{")][-1])

    dirs = {k: os.path.join(tmp_path, k) for k in ("py_on", "cpp_on", "py_off", "cpp_off", "py_never")}
    rep, ctr = run_py(dirs["py_on"], True)
    crep, cctr = run_cpp(dirs["cpp_on"], 1)
    for k in fg.REPORT_KEYS:
        assert rep[0][k] == crep[0][k], k
    fg.compare_directories(dirs["py_on"], dirs["cpp_on"])
    assert ctr == cctr and ctr["stopped_moves"] > 0 and ctr["skipped_sims"] > 0, (ctr, cctr)
    zero = dict.fromkeys(st.COUNTERS, 0)
    assert run_py(dirs["py_off"], False)[1] == zero and run_py(dirs["py_never"], None)[1] == zero
    fg.compare_directories(dirs["py_off"], dirs["py_never"])
    assert run_cpp(dirs["cpp_off"], 0)[1] == zero
    fg.compare_directories(dirs["py_never"], dirs["cpp_off"])
