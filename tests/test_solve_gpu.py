"""az_solve and az_move_quality on the GPU, through the C ABI: values against the independent reference (tests/cpp/solve_ref.cpp), every
output -- node counts and the UNKNOWN set included -- bit for bit against the g++ build of csrc/az_solve.h (tests/cpp/solve_twin.cpp),
independence of the grid and of the order of the positions, the edge positions, the refusals, the move-quality report against a Python
recomputation, purity, and the two Coaches.

Item layout: one item per (position, action), item = 7 * position + action, so a 64-lane wave holds nine positions and one action of the
tenth: n = 9 is the last count that fits one wave (63 items) and n = 10 the first that does not, and both are run."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import feature_gpu as fg
import solve_twin as st

pytestmark = pytest.mark.gpu
N = 300


@pytest.fixture(scope="module")
def positions():
    """The first 300 of the CPU test's positions, rolled so that the first one has, at a budget of 200 nodes, both an action the budget
    cuts and one it does not (with and without a table): the small-budget cases then hold for n = 1 too."""
    pos = st.c4_positions()[:N]
    cut = [st.twin(pos, 0, 200, 0, t)[0] == st.UNKNOWN for t in (0, 8, 12)]
    ok = [i for i in range(N) if all(c[i].any() for c in cut)]
    assert ok
    pos = np.roll(pos, -ok[0], axis=0).copy()
    pos.setflags(write=False)
    return pos


@pytest.fixture(scope="module")
def engine3(engine_mod):
    yield from fg.connect_three_engine(engine_mod)


def test_values_are_the_reference(engine, positions):
    rmv, rv = st.reference(positions, 0)
    mv, v, nodes = engine.solve(positions)
    assert not (mv == st.UNKNOWN).any() and not (v == st.UNKNOWN).any()
    assert np.array_equal(mv, rmv) and np.array_equal(v, rv)
    full = np.array([[(int(a | b) >> (c * 7 + 5)) & 1 for c in range(7)] for a, b in positions], bool)
    assert full.any() and (mv[full] == st.ILLEGAL).all() and (mv[~full] != st.ILLEGAL).all()
    assert set(np.unique(v)) == {-1, 0, 1}


@pytest.mark.parametrize("n", [1, 9, 10, N])
@pytest.mark.parametrize("tt_log2", [0, 8, 12])
@pytest.mark.parametrize("max_nodes", [1 << 20, 200])
def test_bit_exact_against_the_twin(engine, positions, n, tt_log2, max_nodes):
    pos = positions[:n]
    want = st.twin(pos, 0, max_nodes, 0, tt_log2)
    got = engine.solve(pos, max_nodes=max_nodes, tt_log2=tt_log2)
    cut = want[0] == st.UNKNOWN
    if max_nodes == 200:
        assert cut.any() and (~cut & (want[0] != st.ILLEGAL)).any()          # the budget cuts some items and not all
    else:
        assert not cut.any()
    for g, w, name in zip(got, want, ("move_values", "values", "nodes")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    assert np.array_equal(got[0] == st.UNKNOWN, cut)


@pytest.mark.parametrize("max_nodes", [1 << 20, 200])
def test_refill_and_schedule_independence(engine, positions, max_nodes):
    """64 lanes take 2 100 items one after the other, each lane on ONE table slice: the same outputs as the device-sized grid gives, and as
    the reversed order gives, item for item."""
    one_wave = engine.solve(positions, max_nodes=max_nodes, max_lanes=64)
    whole = engine.solve(positions, max_nodes=max_nodes, max_lanes=0)
    rev = engine.solve(positions[::-1].copy(), max_nodes=max_nodes, max_lanes=64)
    for a, b, c in zip(one_wave, whole, rev):
        assert np.array_equal(a, b) and np.array_equal(a, c[::-1])
    again = engine.solve(positions, max_nodes=max_nodes, max_lanes=64)            # the table now holds the first call's entries
    for a, b in zip(one_wave, again):
        assert np.array_equal(a, b)


def test_table_survives_a_change_of_the_grid(engine_mod, positions):
    """The table is kept across calls and a lane's slice must not move with a call's lane count: on ONE fresh engine at tt_log2 8, a call
    of 82 positions (576 lanes), one of 9 (64 lanes), the 82 again, then other positions on 64 lanes and on 1088 -- lane counts 512 and
    1024 apart, whole numbers of 2 KB slices.  Every call's node counts and UNKNOWN sets are the twin's."""
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    try:
        for lo, hi, budget in ((0, 82, 1 << 20), (9, 18, 1 << 20), (0, 82, 1 << 20), (0, 9, 200), (100, 255, 200), (9, 18, 200), (0, 82, 200), (30, 39, 1 << 20)):
            pos = positions[lo:hi]
            want = st.twin(pos, 0, budget, 0, 8)
            got = e.solve(pos, max_nodes=budget, tt_log2=8)
            for g, w, name in zip(got, want, ("move_values", "values", "nodes")):
                assert np.array_equal(g, w), (lo, hi, budget, name)
        for lanes in (64, 576, 64):                              # the same through the cap
            got = e.solve(positions[:200], max_nodes=200, tt_log2=8, max_lanes=lanes)
            want = st.twin(positions[:200], 0, 200, 0, 8)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), lanes
    finally:
        e.close()


def _line(moves):
    s = (0, 0)
    for a in moves:
        s = st.play(*s, a)
    return s


def test_edges(engine, positions):
    won = _line([0, 1, 0, 1, 0, 1, 0])                                   # the first player has four in column 0
    mv, v, nodes = engine.solve(np.array([won], np.uint64))
    assert (mv == st.ILLEGAL).all() and v[0] == 1 and (nodes == 0).all()
    wins = _line([0, 1, 0, 1, 0, 1])                                     # the mover wins at once in column 0; the opponent threatens column 1
    mv, v, nodes = engine.solve(np.array([wins], np.uint64), max_nodes=1000)
    assert mv[0, 0] == 1 and v[0] == 1 and nodes[0, 0] == 0 and (mv[0, 2:] == -1).all() and (nodes[0, 2:] == 1).all()
    assert mv[0, 1] == st.UNKNOWN and nodes[0, 1] == 1000                # the block leaves a seven-stone game: beyond this budget, and +1 wins over it
    two = _line([6, 1, 6, 1, 5, 1, 0, 2, 0, 3])                          # opponent: three in column 1 and 1-2-3 on the bottom row; column 0 is blocked
    tw = st.twin(np.array([two], np.uint64))
    mv, v, nodes = engine.solve(np.array([two], np.uint64))
    assert np.array_equal(mv, tw[0]) and np.array_equal(nodes, tw[2])
    assert v[0] == -1 and (mv[0] == -1).all() and (nodes[0] == 1).all()   # threats in columns 1 and 4: every move loses, each in one node
    # a drawn full board and the position one stone before it, found by playing one of the set's drawn positions out along value-keeping moves
    rmv, rv = st.reference(positions, 0)
    s = tuple(int(x) for x in positions[int(np.flatnonzero(rv == 0)[0])])
    while True:
        m, _ = st.reference(np.array([s], np.uint64), 0)
        nxt = st.play(*s, int(np.flatnonzero(m[0] == 0)[0]))
        if (nxt[0] | nxt[1]) == st.FULL:
            break
        s = nxt
    assert bin(s[0] | s[1]).count("1") == 41
    mv, v, nodes = engine.solve(np.array([s, nxt], np.uint64))
    assert v[0] == 0 and sorted(mv[0]) == [st.ILLEGAL] * 6 + [0] and (nodes[0] == 0).all()       # one empty cell
    assert (mv[1] == st.ILLEGAL).all() and v[1] == 0                                              # the drawn full board
    # min_stones above the positions' counts
    mv, v, nodes = engine.solve(positions[:20], min_stones=42)
    legal = st.twin(positions[:20])[0] != st.ILLEGAL
    assert (mv[legal] == st.UNKNOWN).all() and (mv[~legal] == st.ILLEGAL).all() and (nodes == 0).all() and (v == st.UNKNOWN).all()
    mv, v, nodes = engine.solve(np.zeros((0, 2), np.uint64))
    assert mv.shape == (0, 7) and v.shape == (0,)


def test_connect_three_from_the_empty_board(engine3):
    empty = np.zeros((1, 2), np.uint64)
    want = st.twin(empty, 1)
    got = engine3.solve(empty)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    print("Connect Three, empty board: move values", got[0][0].tolist(), "value", int(got[1][0]), "nodes", got[2][0].tolist())
    assert got[1][0] == 1 and not (got[0] == st.UNKNOWN).any() and got[2].max() > 100000
    pos = st.c3_positions()
    want = st.twin(pos, 1)
    got = engine3.solve(pos)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def _raw_solve(engine, states, n, max_nodes=1 << 20, min_stones=0, tt_log2=12, max_lanes=0, null=()):
    """The C entry with sentinel-filled outputs: (status, outputs)."""
    out = [np.full((max(n, 1), 7), 55, np.int8), np.full(max(n, 1), 55, np.int8), np.full((max(n, 1), 7), 0x55555555, np.uint32)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = engine._lib.az_solve(engine._h, None if "states" in null else p(states), n, max_nodes, min_stones, tt_log2, max_lanes,
                              None if "move_values" in null else p(out[0]), p(out[1]), p(out[2]))
    return rc, out


def test_refusals_write_nothing(engine, positions):
    pos = np.array(positions[:8])

    def refused(*a, **k):
        rc, out = _raw_solve(engine, *a, **k)
        assert rc == fg.AZ_ERR_BAD_ARGUMENT and engine._lib.az_last_error(engine._h).decode().startswith("az_solve")
        assert (out[0] == 55).all() and (out[1] == 55).all() and (out[2] == 0x55555555).all()
    for kw in ({"max_nodes": 0}, {"max_nodes": (1 << 30) + 1}, {"min_stones": -1}, {"min_stones": 43}, {"tt_log2": 7}, {"tt_log2": 17}, {"tt_log2": -1},
               {"max_lanes": 100}, {"max_lanes": -64}, {"null": ("states",)}, {"null": ("move_values",)}):
        refused(pos, 8, **kw)
    refused(pos, -1)
    refused(pos, (1 << 24) + 1)
    for bad in ((1, 1), (1 << 6, 0), (1 << 49, 0), (0, 1 << 1), (1 << 7 | 1 << 9, 0)):       # overlap, row 6, column 7, a floating stone, a gap in a column
        b = pos.copy()
        b[5] = bad
        refused(b, 8)
    engine.selfplay_begin(4, 10, 10, seed=1)
    try:
        refused(pos, 8)
        rc = engine._lib.az_move_quality(engine._h, None, np.zeros(1, np.int32).ctypes.data_as(C.c_void_p), np.zeros(42, np.uint8).ctypes.data_as(C.c_void_p),
                                         1, 1 << 20, 0, 12, 0, np.zeros(42, np.uint8).ctypes.data_as(C.c_void_p), None)
        assert rc == fg.AZ_ERR_BAD_ARGUMENT
    finally:
        engine.selfplay_end()
    rc, out = _raw_solve(engine, pos, 8)
    assert rc == 0 and np.array_equal(out[0], st.twin(pos)[0])


def _recompute_quality(engine, boards, game_len, moves, min_stones, max_nodes):
    n = len(game_len)
    cls, val = np.zeros((n, 42), np.uint8), np.full((n, 42), st.UNKNOWN, np.int8)
    where, reached = [], []
    for g in range(n):
        s = (int(boards[g][0]), int(boards[g][1]))
        for p in range(int(game_len[g])):
            if bin(s[0] | s[1]).count("1") >= min_stones:
                where.append((g, p))
                reached.append(s)
            s = fg.c4_play(s[0], s[1], int(moves[g, p]))
    mv, v, _ = engine.solve(np.array(reached, np.uint64).reshape(-1, 2), max_nodes=max_nodes)
    for (g, p), row, value in zip(where, mv, v):
        cls[g, p] = st.classify(row, int(moves[g, p]))
        val[g, p] = value
    return cls, val


@pytest.mark.parametrize("opening_plies", [0, 6])
def test_move_quality_of_an_arena(engine, opening_plies):
    engine.set_option("arena_opening_plies", opening_plies)
    try:
        out = fg.arena_outputs(engine)
        game_len, moves = out[-2], out[-1]
        boards, ln, _ = engine.arena_get_openings(16)
    finally:
        engine.set_option("arena_opening_plies", 0)
    assert (ln == opening_plies).all()
    top = int(max(bin(int(b[0] | b[1])).count("1") + int(l) for b, l in zip(boards, game_len)))      # the hash nets' games are short
    for min_stones, max_nodes in ((top - 4, 20000), (0, 50), (top - 8, 2000)):
        cls, val = engine.move_quality(game_len, moves, start_boards=boards, max_nodes=max_nodes, min_stones=min_stones)
        wcls, wval = _recompute_quality(engine, boards, game_len, moves, min_stones, max_nodes)
        assert np.array_equal(cls, wcls) and np.array_equal(val, wval)
        print("openings %d, min_stones %d, max_nodes %d: classes %s" % (opening_plies, min_stones, max_nodes, np.bincount(cls.reshape(-1), minlength=6).tolist()))
        assert (cls != st.MQ_SKIPPED).any()
        assert (cls == st.MQ_KEPT).any()                        # a game's winning move, at the least
        if max_nodes == 50:
            assert (cls == st.MQ_UNKNOWN).any()
    if opening_plies == 0:                                     # NULL start boards = the initial board
        a = engine.move_quality(game_len, moves, min_stones=top - 4, max_nodes=2000)
        b = engine.move_quality(game_len, moves, start_boards=boards, min_stones=top - 4, max_nodes=2000)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_move_quality_of_a_hand_written_game(engine, engine_mod):
    """The first player builds three in column 0, passes up the fourth at ply 6 (it plays column 6), and the second player, who has three in
    column 1 by then, wins at ply 7."""
    record = [0, 1, 0, 1, 0, 1, 6, 1]
    moves = np.zeros((1, 42), np.uint8)
    moves[0, :len(record)] = record
    cls, val = engine.move_quality(np.array([len(record)], np.int32), moves, min_stones=6, max_nodes=2000)
    assert cls[0, 6] == st.MQ_WIN_TO_LOSS and val[0, 6] == 1
    assert cls[0, 7] == st.MQ_KEPT and val[0, 7] == 1             # the winner's reply
    assert (cls[0, len(record):] == st.MQ_SKIPPED).all() and (cls[0, :6] == st.MQ_SKIPPED).all()
    for bad_moves, bad_len in (([0, 0, 0, 0, 0, 0, 0], 7), ([7], 1), ([0, 1, 0, 1, 0, 1, 0, 1], 8)):      # a full column, no such column, a move behind the end
        m = np.zeros((1, 42), np.uint8)
        m[0, :len(bad_moves)] = bad_moves
        with pytest.raises(engine_mod.AzError) as ei:
            engine.move_quality(np.array([bad_len], np.int32), m, min_stones=30)
        assert ei.value.status == fg.AZ_ERR_BAD_ARGUMENT
    with pytest.raises(engine_mod.AzError):
        engine.move_quality(np.array([43], np.int32), moves, min_stones=30)


def test_purity(engine, positions):
    before = fg.other_entry_points(engine)
    engine.reset_stats()
    s0 = engine.stats()
    engine.solve(positions, max_nodes=200)
    moves = np.zeros((1, 42), np.uint8)
    engine.move_quality(np.array([4], np.int32), moves + np.arange(42, dtype=np.uint8) % 7, max_nodes=200)
    s1 = engine.stats()
    assert {k: v for k, v in s0.items() if k != "device_ms"} == {k: v for k, v in s1.items() if k != "device_ms"}
    assert s1["device_ms"] > s0["device_ms"]
    fg.assert_same_outputs(fg.other_entry_points(engine), before)


def test_coaches_report_the_same_quality(engine_mod, tmp_path):
    """One iteration on both hosts with solve_min_stones = 26 (C = 128, 32 episodes, as run_coach_pair sizes it): the same twelve counters,
    and checkpoint directories byte-identical to each other and to a Python run with the report off."""
    from alphazero_rs_amd.coach import Coach, QUALITY_KEYS
    Cn, seed = 128, 11
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp", "plain")}

    def run_py(d, min_stones):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=Cn)
        try:
            e.net_init_random(0, 3)
            e.set_option("train_epochs", 1)
            coach = Coach.setup(e, d, 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 1, 32, 25, 1, 1000, 1, log=lambda m: None)
            coach.solve_min_stones = min_stones
            return coach.learn(seed=seed)
        finally:
            e.close()
    rep, plain = run_py(dirs["py"], 26), run_py(dirs["plain"], 0)
    assert "quality" not in plain[0]
    exe = os.path.join(tmp_path, "test_coach_solve")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(fg.ROOT, "include"), os.path.join(fg.ROOT, "tests", "cpp", "test_coach_solve.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, dirs["cpp"], str(Cn), str(seed), "26", str(1 << 20)], check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    crep = json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    assert len(rep) == len(crep) == 1
    for k in fg.REPORT_KEYS:
        assert rep[0][k] == crep[0][k] == plain[0][k], k
    assert rep[0]["quality"] == crep[0]["quality"]
    print("quality", rep[0]["quality"])
    for who in ("new", "old"):
        q = rep[0]["quality"][who]
        assert set(q) == set(QUALITY_KEYS) and q["examined"] == sum(q[k] for k in QUALITY_KEYS[1:])
    assert rep[0]["quality"]["new"]["examined"] > 0 and rep[0]["quality"]["old"]["examined"] > 0
    fg.compare_directories(dirs["py"], dirs["cpp"])
    fg.compare_directories(dirs["py"], dirs["plain"])
