"""Paired arena openings on the CPU: csrc/az_opening.h, the text the arena's opening kernel compiles, built with g++ over the oracle's rules
(tests/cpp/opening_twin.cpp) against a pure-Python restatement of the rule (tests/opening_twin.py), and the properties the rule promises.
No engine and no GPU here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import opening_twin as ot      # noqa: E402

SEEDS = (11, 5)
PLIES = (0, 2, 4, 6, 8, 12)
PAIRS = np.arange(512)

# Bases with exactly 3 and exactly 2 empty cells and no line of three (so none of four) for either side, found by playing random
# non-ending plies from the initial board; (mover's stones, other side's stones).
BASES_3_EMPTY = ((0x285152AA9515, 0x55AAA1454A8A), (0xA81152AA9515, 0x542AA5454AAA))
BASES_2_EMPTY = ((0x18CA63298CA6, 0x653190C65319), (0x9560318CC633, 0x6898C663198C))


def test_header_exists_and_names_its_purpose_word():
    text = open(ot.HEADER).read()
    assert "RNG_OPENING = 7" in text and "hip/" not in text
    assert ot.lib().twin_opening_rng_word() == 7


@pytest.fixture(scope="module")
def grown():
    """(game, seed, n) -> the twin's (boards, len, moves, fallbacks) of pairs 0 .. 511 from the initial board: computed once"""
    return {(g, s, n): ot.grow(g, s, PAIRS, n) for g in (0, 1) for s in SEEDS for n in PLIES}


@pytest.mark.parametrize("game", [0, 1])
def test_twin_equals_the_python_restatement(grown, game):
    for seed in SEEDS:
        for n in PLIES:
            boards, ln, moves, fb = grown[(game, seed, n)]
            for p in PAIRS:
                pb, pl, pm, pf = ot.opening_py(game, seed, int(p), n)
                assert (int(boards[p, 0]), int(boards[p, 1])) == pb, (game, seed, n, p)
                assert ln[p] == pl and moves[p, :pl].tolist() == pm and not moves[p, pl:].any(), (game, seed, n, p)
                assert fb[p] == pf, (game, seed, n, p)


@pytest.mark.parametrize("game", [0, 1])
def test_properties(grown, game):
    k = (4, 3)[game]
    quiet = fell_back = 0
    for seed in SEEDS:
        for i, n in enumerate(PLIES):
            boards, ln, moves, fb = grown[(game, seed, n)]
            assert (ln % 2 == 0).all() and (ln <= n).all()
            assert (ln == n).all()                       # nothing truncates from the initial board for n <= 12
            if i:                                        # the opening with fewer plies is a prefix
                _, ln0, moves0, _ = grown[(game, seed, PLIES[i - 1])]
                for p in PAIRS:
                    assert moves[p, :ln0[p]].tolist() == moves0[p, :ln0[p]].tolist()
            for p in PAIRS:
                s = (int(boards[p, 0]), int(boards[p, 1]))
                assert bin(s[0] | s[1]).count("1") == ln[p] and bin(s[0]).count("1") == bin(s[1]).count("1")    # first seat to move
                assert ot._ended(s, k) == 0 and not ot._line(s[0], k) and not ot._line(s[1], k)                   # never finished
                # replaying the moves from the initial board gives the board
                r = (0, 0)
                for a in moves[p, :ln[p]]:
                    r = ot._play(r, int(a))
                assert r == s
                if fb[p] == 0:
                    quiet += 1
                    assert not ot.win_in_one(s, k), (game, seed, n, p)
                else:
                    fell_back += 1
    # both branches are exercised: Connect Three at n = 6 falls back often, Connect Four rarely
    assert quiet > 1000 and fell_back > (100 if game == 1 else 5), (quiet, fell_back)


def test_connect_three_falls_back_often_at_six_plies(grown):
    fb = grown[(1, 11, 6)][3]
    assert (fb > 0).sum() >= 50 and (fb == 0).sum() >= 50


@pytest.mark.parametrize("game", [0, 1])
def test_truncation(game):
    """3 empty cells: two plies go on, the third would fill the board -> length 2.  2 empty cells: one ply, then the board would be full ->
    the odd ply is dropped, length 0 and the base comes back."""
    for seed in SEEDS:
        for base in BASES_3_EMPTY + BASES_2_EMPTY:
            assert not ot._line(base[0], 3) and not ot._line(base[1], 3) and not (base[0] & base[1])
            empty = 42 - bin(base[0] | base[1]).count("1")
            for n in (2, 4, 12):
                boards, ln, moves, _ = ot.grow(game, seed, np.arange(64), n, base)
                want = 2 if empty == 3 else 0
                assert (ln == want).all(), (base, n)
                assert not moves[:, want:].any()
                for p in range(64):
                    pb, pl, pm, _ = ot.opening_py(game, seed, p, n, base)
                    assert pl == want and (int(boards[p, 0]), int(boards[p, 1])) == pb and moves[p, :pl].tolist() == pm
                if want == 0:
                    assert (boards == np.asarray(base, np.uint64)).all()
                else:
                    assert all(bin(int(x) | int(y)).count("1") == 41 for x, y in boards)


def test_two_plies_cover_all_49_openings():
    boards, ln, moves, _ = ot.grow(0, 11, np.arange(2000), 2)
    assert (ln == 2).all()
    assert len({(int(a), int(b)) for a, b in moves[:, :2]}) == 49
    assert len({(int(a), int(b)) for a, b in boards}) == 49


def test_six_ply_connect_four_openings_are_mostly_quiet():
    """From the initial board, seed 11, pairs 0 .. 1999: a win in one is left in 19 openings (every one through the fallback: the ply before
    made a double threat), against about 10 % for uniform plies."""
    boards, ln, _, fb = ot.grow(0, 11, np.arange(2000), 6)
    hot = [p for p in range(2000) if ot.win_in_one((int(boards[p, 0]), int(boards[p, 1])), 4)]
    assert len(hot) == 19 and all(fb[p] > 0 for p in hot)


def test_pairing_and_book_bases():
    """arena_openings: game g and g + half share pair g % half; with a book the base of pair p is book[p % nb]"""
    book = np.asarray(BASES_3_EMPTY + ((0, 0), (1, 128), (1 | 128, 2 | 256)), np.uint64)
    b, ln, mv = ot.arena_openings(0, 3, 20, 2, book=book)
    assert (b[:10] == b[10:]).all() and (ln[:10] == ln[10:]).all() and (mv[:10] == mv[10:]).all()
    for g in range(20):
        p = g % 10
        pb, pl, pm, _ = ot.opening_py(0, 3, p, 2, tuple(int(x) for x in book[p % 5]))
        assert (int(b[g, 0]), int(b[g, 1])) == pb and ln[g] == pl
    # a shard is a slice of the whole
    bs, ls, ms = ot.arena_openings(0, 3, 20, 2, first=7, n_games=9, book=book)
    assert (bs == b[7:16]).all() and (ls == ln[7:16]).all() and (ms == mv[7:16]).all()
    # seeds 3 and 9: 8 distinct boards for 8 pairs at n = 6 and n = 4 (what the GPU tests rely on)
    for seed in (3, 9):
        for n in (6, 4):
            b, _, _ = ot.arena_openings(0, seed, 16, n)
            assert len({(int(x), int(y)) for x, y in b[:8]}) == 8, (seed, n)
