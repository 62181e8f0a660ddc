"""The 40 fresh roots of the decided-move stop's tests (tests/test_search_stop_cpu.py checks their properties, tests/test_search_stop_gpu.py
searches them): the empty board, a root with an immediate win, a root with exactly one legal move, a near-full board and 36 positions of
random play, each (mover's stones, the other side's stones) as the engine packs a canonical board.  TEST INFRASTRUCTURE ONLY."""
import stop_twin as st

EMPTY, WIN, ONE_MOVE, NEAR_FULL = 0, 1, 2, 3
ROOTS = [
    (0x0, 0x0),
    (0x7, 0x380),
    (0x590a6e71589, 0x386b5108ca36),
    (0x545180e75a0b, 0xa8aa77088594),
    (0x20208703, 0xc001001408c),
    (0x80001400001, 0x40000a0c000),
    (0x1c1811020001, 0x2e1c082),
    (0x20a28081, 0x1850414000),
    (0x80810004005, 0x140000e00082),
    (0x80840000080, 0x40030004001),
    (0xc0850000003, 0x10a000c084),
    (0x30000000, 0x40800004000),
    (0xc2000208001, 0x5800404180),
    (0x83030000109, 0x40800604096),
    (0x30001042c082, 0xc0800250105),
    (0x180070000002, 0x240800200081),
    (0xc0800400180, 0x1010204203),
    (0x1c1820a00500, 0x20201041c283),
    (0x8005160810d, 0x438a0814092),
    (0x820200486, 0x1010404b01),
    (0x80093a08503, 0x14006440429c),
    (0x0, 0x1),
    (0x800038080, 0x41030004001),
    (0x4100, 0x800000081),
    (0xc082000dc01, 0x1000d0200386),
    (0x4003, 0x810000080),
    (0x1820024001, 0x50218080),
    (0x10200000, 0xc00000),
    (0x140020018081, 0x80810024006),
    (0x50080060c206, 0xac0070000581),
    (0x800004080, 0x40000200003),
    (0x40000000000, 0x80000000080),
    (0x810000000, 0x200080),
    (0x42000004000, 0x1800000180),
    (0x82010018080, 0x141820204000),
    (0x4500140c114, 0x2800a300ab),
    (0x4000, 0x40800000000),
    (0x382030004000, 0x418c0208080),
    (0x30000501, 0x40040004282),
    (0x4000, 0x800000000),
]


def twin_runs(net_kind, salt, budget, roots=None):
    """The simulations the twin runs on each root, built fresh, at temperature 0 with the rule on."""
    out = []
    for r in (ROOTS if roots is None else roots):
        t = st.Tree(budget, net_kind=net_kind, salt=salt, root=r)
        out.append(t.get_action_prob(r[0], r[1], 0.0, seed=5, game_id=9)[3])
        t.close()
    return out


def twin_stopped(net_kind, salt, budget):
    return sum(1 for x in twin_runs(net_kind, salt, budget) if x < budget)
