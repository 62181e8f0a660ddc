"""Paired arena openings on the GPU ("arena_opening_plies" / az_arena_set_opening_book / az_arena_get_openings, include/az_engine.h): the
device's openings against the g++ build of csrc/az_opening.h (tests/opening_twin.py), every game against the oracle and against the
contract -- game g IS the sharded single-game call from start_board = opening(g) with the feature off: result, move record and eval log --
shards, the book, the refusals, the off state, and both Coaches."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg       # noqa: E402
import opening_twin as ot      # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_SALT = fg.MODEL_SALT
KEY = "arena_opening_plies"
LOG_CAP = 21 * 51 + 8          # records per game and player: at most 21 moves of 50 simulations + a root each


@pytest.fixture
def off(engine):
    """the session engine with the feature off before and after the test"""
    engine.set_arena_openings(0)
    engine.arena_set_opening_book(None)
    yield engine
    engine.set_arena_openings(0)
    engine.arena_set_opening_book(None)


def _hash_pair(e, engine_mod, new_id, old_id, salt):
    """hash nets that are the oracle's HashNet(salt) with new_model_id = 0, old_model_id = 1"""
    e.net_set_kind(new_id, engine_mod.NET_HASH, salt - new_id * MODEL_SALT)
    e.net_set_kind(old_id, engine_mod.NET_HASH, salt + MODEL_SALT - old_id * MODEL_SALT)


def _logs(e, n, cap):
    out = []
    for which in (0, 1):
        cnt, states, pis, vs = e.arena_get_evals(which, n, cap)
        assert cnt.max() <= cap
        out.append([(int(cnt[g]), states[g, :cnt[g]].copy(), pis[g, :cnt[g]].view(np.uint32).copy(), vs[g, :cnt[g]].view(np.uint32).copy())
                    for g in range(n)])
    return out


def _play(e, total, sims, plies, book=None, cap=LOG_CAP, first=0, n=None, **kw):
    """one arena call with the feature set as given: results, openings, move record, eval logs of its games"""
    e.set_arena_openings(plies)
    e.arena_set_opening_book(book)
    try:
        n = total if n is None else n
        sharded = dict(first_game=first, total_games=total) if (first or n != total) else {}
        wld, res = e.arena(n, sims, record_evals=cap, **sharded, **kw)
        boards, ln, mv = e.arena_get_openings(n)
        glen, gmoves = e.arena_get_moves(n)
        return dict(wld=wld, res=res, boards=boards, len=ln, moves=mv, glen=glen, gmoves=gmoves, logs=_logs(e, n, cap) if cap else None)
    finally:
        e.set_arena_openings(0)
        e.arena_set_opening_book(None)


def _assert_contract(e, got, total, sims, cap=LOG_CAP, first=0, **kw):
    """every game of `got` is the single-game sharded call from its opening with the feature off"""
    wld, seen = np.zeros(3, np.uint64), [0, 0]
    for i in range(len(got["res"])):
        g = first + i
        w, r = e.arena(1, sims, first_game=g, total_games=total, start_board=tuple(int(x) for x in got["boards"][i]), record_evals=cap, **kw)
        wld += w
        assert r[0] == got["res"][i], g
        glen, gmoves = e.arena_get_moves(1)
        assert glen[0] == got["glen"][i] and np.array_equal(gmoves[0], got["gmoves"][i]), g
        b, ln, _ = e.arena_get_openings(1)                    # feature off: the common start position, no random ply
        assert np.array_equal(b[0], got["boards"][i]) and ln[0] == 0
        ref = _logs(e, 1, cap)
        for which in (0, 1):
            a, b = got["logs"][which][i], ref[which][0]
            assert a[0] == b[0], (g, which)                   # (0 records: the game ended before this player's first move)
            assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), (g, which)
            seen[which] += a[0]
    assert wld.tolist() == got["wld"].tolist()
    assert seen[0] > 0 and seen[1] > 0                        # both players' logs were compared


def _assert_twin(got, game, seed, total, plies, first=0, book=None, start_board=None):
    b, ln, mv = ot.arena_openings(game, seed, total, plies, first=first, n_games=len(got["res"]), book=book, start_board=start_board)
    assert np.array_equal(got["boards"], b) and np.array_equal(got["len"], ln) and np.array_equal(got["moves"], mv)


@pytest.mark.parametrize("seed,plies", [(3, 6), (9, 4)])
def test_device_openings_match_the_twin(off, engine_mod, seed, plies):
    e = off
    _hash_pair(e, engine_mod, 81, 80, 2468)
    got = _play(e, 16, 25, plies, new_model_id=81, old_model_id=80, seed=seed, cap=0)
    _assert_twin(got, 0, seed, 16, plies)
    assert (got["len"] == plies).all()
    assert np.array_equal(got["boards"][:8], got["boards"][8:]) and np.array_equal(got["moves"][:8], got["moves"][8:])
    assert len({tuple(x) for x in got["boards"][:8].tolist()}) == 8                   # one position per pair, all different
    # the move record and game_len hold only the plies the models played: replayed from the opening they end the game as reported
    for g in range(16):
        s, player, k = tuple(int(x) for x in got["boards"][g]), 1, 4
        assert got["glen"][g] >= 1 and got["glen"][g] + plies <= 42
        for j in range(got["glen"][g]):
            assert ot._ended(s, k) == 0
            s, player = ot._play(s, int(got["gmoves"][g, j])), -player
        end = ot._ended(s, k)
        assert end != 0 and got["res"][g] == (0 if end == "draw" else -player)


def test_every_game_matches_the_oracle(off, oracle, engine_mod):
    e = off
    _hash_pair(e, engine_mod, 83, 82, 1357)
    e.reset_stats()
    got = _play(e, 16, 50, 4, new_model_id=83, old_model_id=82, seed=3, cap=0)
    _assert_twin(got, 0, 3, 16, 4)
    st = e.stats()
    assert st["games"] == 16 and st["simulations"] == 50 * int(got["glen"].sum())    # az_stats: the models' plies only, no opening ply
    tally = np.zeros(3, np.uint64)
    for g in range(16):
        w, r, _ = oracle.arena_ex(16, 50, first_game=g, n_games=1, net_kind=oracle.NET_HASH, salt=1357, seed=3, new_model_id=0, old_model_id=1,
                                  start_board=got["boards"][g])
        assert r[0] == got["res"][g], g
        tally += w
    assert tally.tolist() == got["wld"].tolist() and int(tally.sum()) == 16


def test_contract_hash_nets(off, engine_mod):
    e = off
    _hash_pair(e, engine_mod, 85, 84, 97531)
    kw = dict(new_model_id=85, old_model_id=84, seed=9)
    got = _play(e, 16, 50, 6, **kw)
    _assert_twin(got, 0, 9, 16, 6)
    _assert_contract(e, got, 16, 50, **kw)


def test_contract_two_simulations_in_flight(off, engine_mod):
    e = off
    _hash_pair(e, engine_mod, 85, 84, 97531)
    kw = dict(new_model_id=85, old_model_id=84, seed=3, num_sim_threads=2)
    got = _play(e, 16, 50, 4, **kw)
    _assert_contract(e, got, 16, 50, **kw)


@pytest.fixture(scope="module")
def conv_engine(engine_mod):
    """two randomly initialised conv models (ids 1 and 0) at the smallest width the suite uses"""
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    e.net_init_random(0, 3)
    e.net_init_random(1, 4)
    yield e
    e.close()


def test_contract_conv_models(conv_engine):
    kw = dict(new_model_id=1, old_model_id=0, seed=9)
    got = _play(conv_engine, 16, 25, 6, **kw)
    _assert_twin(got, 0, 9, 16, 6)
    _assert_contract(conv_engine, got, 16, 25, **kw)


def test_a_different_game_per_pair(conv_engine):
    """THE POINT OF THE FEATURE: a conv net is a function of the state and the arena plays at temperature 0, so from one position a seating
    is one game; with six-ply openings there are at least as many different games as pairs."""
    got = _play(conv_engine, 16, 25, 6, cap=0, new_model_id=1, old_model_id=0, seed=3)
    records = {(tuple(got["boards"][g].tolist()), tuple(got["gmoves"][g, :got["glen"][g]].tolist())) for g in range(16)}
    assert len(records) >= 8, len(records)


def test_contract_connect_three(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128, game=1)
    try:
        _hash_pair(e, engine_mod, 11, 10, 8642)
        kw = dict(new_model_id=11, old_model_id=10, seed=3)
        got = _play(e, 16, 50, 6, **kw)
        _assert_twin(got, 1, 3, 16, 6)
        _assert_contract(e, got, 16, 50, **kw)
    finally:
        e.close()


def test_shards_add_up(off, engine_mod):
    e = off
    _hash_pair(e, engine_mod, 87, 86, 1212)
    kw = dict(new_model_id=87, old_model_id=86, seed=9)
    whole = _play(e, 16, 25, 6, cap=0, **kw)
    parts = [_play(e, 16, 25, 6, cap=0, first=lo, n=hi - lo, **kw) for lo, hi in ((0, 5), (5, 16))]
    for k in ("res", "boards", "len", "moves", "glen", "gmoves"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    assert (parts[0]["wld"] + parts[1]["wld"]).tolist() == whole["wld"].tolist()
    _assert_twin(parts[1], 0, 9, 16, 6, first=5)


def test_opening_book(off, oracle, engine_mod):
    e = off
    _hash_pair(e, engine_mod, 89, 88, 3434)
    book = []
    for line in ((3, 3), (0, 6), (2, 4, 4, 2), (3, 2, 3, 2, 1, 1), ()):
        s = (0, 0)
        for a in line:
            s = oracle.c4_play(s[0], s[1], a)
        book.append(s)
    book = np.asarray(book, np.uint64)
    kw = dict(new_model_id=89, old_model_id=88, seed=3)
    got = _play(e, 20, 25, 0, book=book, **kw)
    assert (got["len"] == 0).all()
    for g in range(20):
        assert np.array_equal(got["boards"][g], book[(g % 10) % 5]), g
    _assert_contract(e, got, 20, 25, **kw)
    # a book plus two plies: two random plies onto each entry
    got2 = _play(e, 20, 25, 2, book=book, cap=0, **kw)
    _assert_twin(got2, 0, 3, 20, 2, book=book)
    assert (got2["len"] == 2).all()
    for g in range(20):
        s = tuple(int(x) for x in book[(g % 10) % 5])
        for a in got2["moves"][g, :2]:
            s = oracle.c4_play(s[0], s[1], int(a))
        assert s == tuple(int(x) for x in got2["boards"][g])
    assert len({tuple(x) for x in got2["boards"][:10].tolist()}) > 5                  # pairs p and p + 5 share an entry, not an opening


def test_off_is_off(off, engine_mod):
    e = off
    _hash_pair(e, engine_mod, 91, 90, 5656)
    kw = dict(new_model_id=91, old_model_id=90, seed=9)
    fresh = engine_mod.Engine(device=0, max_batch=256, net_channels=128)           # never saw the keys
    try:
        _hash_pair(fresh, engine_mod, 91, 90, 5656)
        w0, r0 = fresh.arena(16, 25, **kw)
        l0, m0 = fresh.arena_get_moves(16)
        b0, n0, v0 = fresh.arena_get_openings(16)
        assert not b0.any() and not n0.any() and not v0.any()
    finally:
        fresh.close()
    for prepare in (lambda: None, lambda: (e.set_arena_openings(6), e.arena_set_opening_book([(1, 128)]), e.set_arena_openings(0),
                                            e.arena_set_opening_book(None))):
        prepare()
        w, r = e.arena(16, 25, **kw)
        l, m = e.arena_get_moves(16)
        assert w.tolist() == w0.tolist() and np.array_equal(r, r0) and np.array_equal(l, l0) and np.array_equal(m, m0)
    sb = (1 | (1 << 7), (1 << 1) | (1 << 14))
    w, r = e.arena(4, 25, start_board=sb, **kw)
    b, n, _ = e.arena_get_openings(4)
    assert (b == np.asarray(sb, np.uint64)).all() and not n.any()


def test_refusals(off, engine_mod, oracle):
    e = off
    for bad in (3, 14, -2, 1, 13):
        with pytest.raises(engine_mod.AzError) as ei:
            e.set_option(KEY, bad)
        assert ei.value.status == 1
    good = np.asarray([(1, 128)], np.uint64)
    e.arena_set_opening_book(good)
    won = (0, 0)
    for a in (0, 1, 0, 1, 0, 1, 6, 1):                 # the second mover completes column 1
        won = oracle.c4_play(won[0], won[1], a)
    assert oracle.c4_ended(*won) != 0.0
    for bad in ([(3, 1)], [(1, 128), (1 << 6, 0)], [(1, 128), won], np.zeros((65537, 2), np.uint64)):
        with pytest.raises(engine_mod.AzError) as ei:
            e.arena_set_opening_book(bad)
        assert ei.value.status == 1
    e.arena_set_opening_book(np.zeros((65536, 2), np.uint64))                      # the largest book
    e.arena_set_opening_book(good)
    _hash_pair(e, engine_mod, 93, 92, 7878)
    with pytest.raises(engine_mod.AzError) as ei:                                   # a book combined with use_start_board
        e.arena(4, 10, new_model_id=93, old_model_id=92, start_board=(1, 128))
    assert ei.value.status == 1
    w, _ = e.arena(4, 10, new_model_id=93, old_model_id=92)                         # a refused book left the previous one in place
    b, _, _ = e.arena_get_openings(4)
    assert (b == good).all() and int(w.sum()) == 4
    fresh = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    try:
        with pytest.raises(engine_mod.AzError) as ei:                               # no arena yet
            fresh.arena_get_openings(4)
        assert ei.value.status == 1
    finally:
        fresh.close()


def test_python_and_cpp_coach_agree_with_arena_openings(engine_mod, tmp_path):
    """tests/test_coach_gpu.py::test_python_and_cpp_coach_agree with Coach.arena_opening_plies set on both hosts: byte-identical files; the
    option is on for the gate and off again behind it."""
    seen = []

    def configure(coach, e):
        coach.arena_opening_plies = 4
        orig = e.set_option

        def spy(key, value):
            if key == KEY:
                seen.append((key, value, e.arena_get_openings(8)[1].tolist() if seen else None))   # behind the gate: its games' openings
            return orig(key, value)
        e.set_option = spy

    def inspect(e):
        del e.set_option                                 # the spy: the class's method again
        # on before the gate, off behind it -- and the gate's eight games were played from four-ply openings
        assert seen == [(KEY, 4, None), (KEY, 0, [4] * 8)], seen
        e.net_init_random(5, 1)
        e.arena(4, 10, new_model_id=5, old_model_id=5)
        assert not e.arena_get_openings(4)[1].any()                                # the option is at 0 after learn()
    fg.run_coach_pair(engine_mod, tmp_path, ["arena_opening_plies=4"], configure, inspect=inspect)
