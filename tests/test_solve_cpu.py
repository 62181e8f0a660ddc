"""csrc/az_solve.h on the host (tests/cpp/solve_twin.cpp, the text the kernels compile) against an independent memoised full minimax
(tests/cpp/solve_ref.cpp): every legal root move of 2 000 random-play Connect Four positions with 26 to 41 stones and of 300 Connect Three
positions, with and without the transposition table, at max_nodes = 2^20.  No item may be UNKNOWN and every value is the reference's.
Then the values[i] combination rule under a budget small enough to cut siblings, and a sanitizer build of the twin as a stand-alone program."""
import numpy as np
import pytest

import solve_twin as st


@pytest.mark.parametrize("tt_log2", [0, 12])
def test_connect_four_values_are_the_reference(tt_log2):
    pos = st.c4_positions()
    stones = np.array([bin(int(a | b)).count("1") for a, b in pos])
    assert stones.min() == 26 and stones.max() == 41 and len(pos) == 2000
    rmv, rv = st.c4_reference()
    mv, v, nodes = st.twin(pos, 0, 1 << 20, 0, tt_log2)
    print("tt_log2 %d: items %d, nodes mean %.1f max %d" % (tt_log2, int((mv != st.ILLEGAL).sum()), nodes.mean(), nodes.max()))
    assert not (mv == st.UNKNOWN).any() and not (v == st.UNKNOWN).any()
    assert (mv == st.ILLEGAL).any()                       # full columns are among them
    assert np.array_equal(mv, rmv) and np.array_equal(v, rv)
    assert set(np.unique(rv)) == {-1, 0, 1}
    assert nodes.max() > 1000 and (nodes[mv == st.ILLEGAL] == 0).all()


@pytest.mark.parametrize("tt_log2", [0, 12])
def test_connect_three_values_are_the_reference(tt_log2):
    pos = st.c3_positions()
    assert len(pos) == 300 and min(bin(int(a | b)).count("1") for a, b in pos) >= 8
    rmv, rv = st.c3_reference()
    mv, v, nodes = st.twin(pos, 1, 1 << 20, 0, tt_log2)
    assert not (mv == st.UNKNOWN).any()
    assert np.array_equal(mv, rmv) and np.array_equal(v, rv)


def test_connect_three_below_sixteen_stones():
    """A handful of Connect Three positions with 10 to 14 stones against the reference, which needs seconds for each of them."""
    pos = st.c3_low_positions()
    stones = [bin(int(a | b)).count("1") for a, b in pos]
    assert min(stones) >= 10 and max(stones) <= 14
    rmv, rv = st.reference(pos, 1)
    for tt_log2 in (0, 12):
        mv, v, _ = st.twin(pos, 1, 1 << 20, 0, tt_log2)
        assert not (mv == st.UNKNOWN).any() and np.array_equal(mv, rmv) and np.array_equal(v, rv)


def test_the_table_changes_node_counts_only():
    pos = st.c4_positions()[:400]
    a, b = st.twin(pos, 0, 1 << 20, 0, 0), st.twin(pos, 0, 1 << 20, 0, 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert b[2].sum() < a[2].sum()


def test_items_do_not_depend_on_their_neighbours():
    """One table slice serves every item in turn: an item's value and node count are those of the item run alone."""
    pos = st.c4_positions()[:300]
    mv, v, nodes = st.twin(pos, 0, 200, 0, 8)
    rmv, rv, rnodes = st.twin(pos[::-1], 0, 200, 0, 8)
    assert np.array_equal(mv, rmv[::-1]) and np.array_equal(v, rv[::-1]) and np.array_equal(nodes, rnodes[::-1])
    for i in (0, 17, 123):
        one = st.twin(pos[i:i + 1], 0, 200, 0, 8)
        assert np.array_equal(one[0][0], mv[i]) and np.array_equal(one[2][0], nodes[i])


def test_values_combination_rule_under_a_small_budget():
    """values[i] = +1 if any action is +1, else UNKNOWN if any legal action is UNKNOWN, else the maximum: a budget of 30 nodes without a
    table cuts many siblings of the deepest positions, among them siblings of a winning move."""
    pos = st.c4_positions()
    mv, v, nodes = st.twin(pos, 0, 30, 0, 0)
    full = st.c4_reference()[0]
    cut = mv == st.UNKNOWN
    assert cut.any() and not cut.all(axis=1).all()
    assert (nodes[cut] == 30).all() and (nodes[~cut] <= 30).all()
    assert np.array_equal(mv[~cut], full[~cut])                   # what the budget did not cut is exact
    want = np.array([st.combine(row) for row in mv], np.int8)
    assert np.array_equal(v, want)
    win_beats_unknown = cut.any(axis=1) & (mv == 1).any(axis=1)
    unknown_wins = cut.any(axis=1) & ~(mv == 1).any(axis=1)
    assert win_beats_unknown.sum() > 0 and unknown_wins.sum() > 0
    assert (v[win_beats_unknown] == 1).all() and (v[unknown_wins] == st.UNKNOWN).all()


def test_min_stones_and_finished_positions():
    pos = st.c4_positions()[:50]
    mv, v, nodes = st.twin(pos, 0, 1 << 20, 42, 12)
    legal = st.c4_reference()[0][:50] != st.ILLEGAL
    assert (mv[legal] == st.UNKNOWN).all() and (mv[~legal] == st.ILLEGAL).all() and (nodes == 0).all() and (v == st.UNKNOWN).all()
    won = (0, 0)
    for a in (0, 1, 0, 1, 0, 1, 0):                               # the first player stacks four in column 0
        won = st.play(*won, a)
    mv, v, nodes = st.twin(np.array([won], np.uint64), 0, 1 << 20, 0, 12)
    assert (mv == st.ILLEGAL).all() and v[0] == 1 and (nodes == 0).all()      # the value as the tree sees it: to the side that moved in
    rmv, rv = st.reference(np.array([won], np.uint64), 0)
    assert np.array_equal(mv, rmv) and np.array_equal(v, rv)


def test_header_classify_and_combine():
    """solve_classify / solve_combine of csrc/az_solve.h (the g++ build) on hand-written rows, then on every row of {-1, 0, +1, UNKNOWN,
    ILLEGAL}^4 (padded with ILLEGAL) and every legal action of it against the restatement the GPU tests recompute with."""
    U, I = st.UNKNOWN, st.ILLEGAL
    rows = [([1, U, 0, I, -1, U, 0], 0, st.MQ_KEPT, 1), ([1, U, 0, I, -1, U, 0], 1, st.MQ_UNKNOWN, 1), ([1, U, 0, I, -1, U, 0], 2, st.MQ_WIN_TO_DRAW, 1),
            ([1, 0, 0, I, -1, 0, 0], 4, st.MQ_WIN_TO_LOSS, 1), ([0, 0, -1, I, -1, 0, 0], 2, st.MQ_DRAW_TO_LOSS, 0), ([0, 0, -1, I, -1, 0, 0], 0, st.MQ_KEPT, 0),
            ([-1, -1, -1, I, I, I, I], 1, st.MQ_KEPT, -1), ([0, U, -1, I, I, I, I], 0, st.MQ_UNKNOWN, U), ([0, U, -1, I, I, I, I], 2, st.MQ_UNKNOWN, U)]
    cls, val = st.header_classify([r[0] for r in rows], [r[1] for r in rows])
    assert cls.tolist() == [r[2] for r in rows] and val.tolist() == [r[3] for r in rows]
    import itertools
    allrows, acts = [], []
    for combo in itertools.product((-1, 0, 1, U, I), repeat=4):
        for a in range(4):
            if combo[a] != I:
                allrows.append(list(combo) + [I, I, I])
                acts.append(a)
    cls, val = st.header_classify(allrows, acts)
    assert cls.tolist() == [st.classify(np.array(r, np.int8), a) for r, a in zip(allrows, acts)]
    assert val.tolist() == [st.combine(np.array(r, np.int8)) for r in allrows]
    assert set(cls.tolist()) == {st.MQ_KEPT, st.MQ_WIN_TO_DRAW, st.MQ_WIN_TO_LOSS, st.MQ_DRAW_TO_LOSS, st.MQ_UNKNOWN}


def test_coach_tally_seats_and_movers():
    """coach.quality_tally: the new model holds the first seat in the games below total // 2, the first seat moves at the even plies."""
    from alphazero_rs_amd.coach import quality_tally
    cls = np.zeros((4, 42), np.uint8)
    cls[0, 30], cls[0, 31] = st.MQ_KEPT, st.MQ_WIN_TO_LOSS             # global game 2 of 8: new is first -> ply 30 new, ply 31 old
    cls[3, 30], cls[3, 33] = st.MQ_DRAW_TO_LOSS, st.MQ_UNKNOWN         # global game 5 of 8: old is first -> ply 30 old, ply 33 new
    got = quality_tally(cls, first_game=2, total_games=8)
    assert got.dtype == np.uint64 and got.tolist() == [[2, 1, 0, 0, 0, 1], [2, 0, 0, 1, 1, 0]]
    assert quality_tally(np.zeros((0, 42), np.uint8), 0, 0).tolist() == [[0] * 6, [0] * 6]


def test_twin_under_the_host_sanitizers():
    """The search as a stand-alone g++ program under AddressSanitizer and UBSan: same output, no report (a report aborts the program)."""
    pos = st.c4_positions()[:200]
    plain = st.twin(pos, 0, 5000, 0, 8)
    san = st.twin(pos, 0, 5000, 0, 8, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for a, b in zip(plain, san):
        assert np.array_equal(a, b)
