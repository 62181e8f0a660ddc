"""The decided-move stop without a GPU (include/az_search_stop.h, csrc/az_stop.h): the predicate in its g++ build
against brute force, the twin (tests/cpp/stop_twin.cpp) against the unchanged oracle on fresh roots, the input conditions of the GPU tests
(tests/test_search_stop_gpu.py), and where the new surface sits: an extension header, a typed setter, a Python list of its own."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stop_twin as st      # noqa: E402

HASH_SALT = 1234
SYMBOLS = ["az_search_stop_set", "az_search_stop_get", "az_search_stop_stats"]


# ---- the predicate ------------------------------------------------------------------------------------------------------------------------
def _arg_max_can_change(counts, left):
    """Brute force: some way of handing out `left` unit increments changes the SET of maximal children."""
    top = lambda c: frozenset(i for i, x in enumerate(c) if x == max(c))
    now = top(counts)
    for extra in itertools.combinations_with_replacement(range(len(counts)), left):
        c = list(counts)
        for i in extra:
            c[i] += 1
        if top(c) != now:
            return True
    return False


def test_predicate_against_brute_force():
    """Every count vector of 1 .. 4 children with counts 0 .. 6 and every left 0 .. 6.  With two or more children and simulations still to
    come, decided holds iff no hand-out of `left` unit increments changes the set of maximal children.  The rule as csrc/az_stop.h states it
    is deliberately narrower in two corners, which are held to their own statement: a single child counts against a runner-up of 0 (decided
    iff n > left, although its arg-max cannot change), and with left = 0 the strict inequality asks for a unique maximum (decided iff
    n1 > n2, although nothing can change any more; the kernels never ask with left = 0).  Everywhere decided implies that the arg-max
    cannot change."""
    checked = held = 0
    for nchild in range(1, 5):
        for counts in itertools.product(range(7), repeat=nchild):
            for left in range(7):
                fixed = not _arg_max_can_change(counts, left)
                got = st.decided(counts, left)
                assert got == st.decided_py(counts, left), (counts, left)
                if nchild == 1:
                    assert got == (counts[0] > left), (counts, left)
                elif left == 0:
                    top = sorted(counts, reverse=True)
                    assert got == (top[0] > top[1]), (counts, left)
                else:
                    assert got == fixed, (counts, left)
                assert fixed or not got, (counts, left)
                checked += 1
                held += got
    assert checked == (7 + 49 + 343 + 2401) * 7 and 0 < held < checked


def test_word_layout():
    """csrc/az_stop.h's word: bit 0 searches, bits 1 .. 29 the simulations left, bit 30 decided, bit 31 eligible; the playout cap's own word
    (1 | left << 1) is the same word with the upper bits clear."""
    L = st.lib()
    for budget in (0, 1, 8, 32, 400, 65535):
        for elig in (0, 1):
            w = L.stop_twin_word(budget, elig)
            assert w == (1 | budget << 1 | (elig << 31)) and L.stop_twin_left(w) == budget
            assert L.stop_twin_left(w | 1 << 30) == budget
    assert L.stop_twin_eligible(3, 4) == 1 and L.stop_twin_eligible(2, 4) == 0          # ply + 1 >= temp_threshold
    assert L.stop_twin_eligible(0, -2 ** 31) == 1 and L.stop_twin_eligible(41, 2 ** 31 - 1) == 0


# ---- the twin against the oracle ------------------------------------------------------------------------------------------------------------
B = 32


def _fresh(oracle, net_kind, salt, root):
    """(counts, q) of the oracle's Tree(sims = k) built at `root` for k = 0 .. B, and its pi at B."""
    rows = []
    for k in range(B + 1):
        t = oracle.Tree(k, net_kind=net_kind, salt=salt, root=root, reserve=st.default_reserve(B))
        pi, counts, q = t.get_action_prob(root[0], root[1], 0.0, seed=5, game_id=9)
        t.close()
        rows.append((pi, counts, q))
    return rows


@pytest.mark.parametrize("net", ["stub", "hash"])
def test_twin_against_oracle_on_fresh_roots(oracle, net):
    """32 simulations at temperature 0: a stopped move's counts and q are Tree(sims = i*)'s, its pi is Tree(sims = 32)'s, the rule holds at
    i* and fails at every smaller i (taken from the oracle's own counts)."""
    import search_stop_roots as roots
    net_kind, salt = (oracle.NET_STUB, 0) if net == "stub" else (oracle.NET_HASH, HASH_SALT)
    stopped = 0
    for root in roots.ROOTS[:12]:
        want = _fresh(oracle, net_kind, salt, root)
        t = st.Tree(B, net_kind=net_kind, salt=salt, root=root)
        pi, counts, q, ran = t.get_action_prob(root[0], root[1], 0.0, seed=5, game_id=9)
        t.close()
        assert int(counts.sum()) == ran                                   # a fresh root: i* = sum(counts)
        assert np.array_equal(counts, want[ran][1]) and np.array_equal(q.view(np.uint32), want[ran][2].view(np.uint32))
        assert np.array_equal(pi, want[B][0]) and pi.max() == 1.0 and pi.sum() == 1.0
        nz = lambda c: [int(x) for x, v in zip(c, _valid(oracle, root)) if v]
        for i in range(ran):
            assert not st.decided_py(nz(want[i][1]), B - i), (root, i)
        if ran < B:
            assert st.decided_py(nz(want[ran][1]), B - ran)
            stopped += 1
        assert int(t.ctr[0]) == 1 and int(t.ctr[1]) == (ran < B) and int(t.ctr[2]) == B and int(t.ctr[3]) == B - ran
    assert stopped >= 4, stopped


def _valid(oracle, root):
    m = oracle.c4_valid_mask(root[0], root[1])
    return [(m >> a) & 1 for a in range(7)]


def test_input_condition_of_the_fresh_root_gpu_test():
    """tests/test_search_stop_gpu.py's 40 roots: they include the empty board, an immediate win, a single legal move and a near-full
    board, and the twin alone stops at least half of the hash-net trees at B = 32."""
    import search_stop_roots as roots
    assert len(roots.ROOTS) == 40 and len(set(roots.ROOTS)) == 40
    assert roots.ROOTS[roots.EMPTY] == (0, 0)
    pop = lambda x: bin(x).count("1")
    from oracle import oracle_py
    assert pop(oracle_py.c4_valid_mask(*roots.ROOTS[roots.ONE_MOVE])) == 1
    assert pop(roots.ROOTS[roots.NEAR_FULL][0] | roots.ROOTS[roots.NEAR_FULL][1]) >= 38
    win = roots.ROOTS[roots.WIN]
    assert any(oracle_py.c4_ended(*oracle_py.c4_play(win[0], win[1], a)) != 0.0 for a in range(7) if (oracle_py.c4_valid_mask(*win) >> a) & 1)
    for r in roots.ROOTS:
        assert oracle_py.c4_ended(r[0], r[1]) == 0.0
    assert roots.twin_stopped(st.NET_HASH, HASH_SALT + 10 * 0x51ED27, B) >= 20


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------
def _strip(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_header_is_an_extension_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "az_search_stop.h")).read()
    code = _strip(hdr)
    assert '#include "az_engine.h"' in code
    assert sorted(re.findall(r"\baz_status\s+(az_\w+)\s*\(", code)) == sorted(SYMBOLS)
    src = os.path.join(tmp_path, "use.c")
    with open(src, "w") as f:
        f.write('#include "az_search_stop.h"\nint main(void) { az_status (*f)(az_engine*, int32_t) = az_search_stop_set; uint64_t o[4]; return f(0, 2) == az_search_stop_stats(0, o, 0); }\n')
    for cc, flags in (("gcc", ["-std=c99"]), ("g++", ["-std=c++17", "-x", "c++"])):
        subprocess.check_call([cc, *flags, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src])
    engine_h = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    assert "search_stop" not in engine_h


def test_python_list_and_exports(engine_mod):
    assert engine_mod.SEARCH_STOP_EXPORTS == SYMBOLS
    for s in SYMBOLS:
        assert s not in engine_mod.EXPORTS and s not in engine_mod.EXT_EXPORTS
    assert engine_mod.EXT_EXPORTS == ["az_reanalyse"]
    for path in (engine_mod.LIB_PATH, engine_mod.DIAG_LIB_PATH):
        lib = ctypes.CDLL(path)
        for s in SYMBOLS:
            assert hasattr(lib, s), (path, s)
    for m in ("set_search_stop", "get_search_stop", "search_stop_stats"):
        assert hasattr(engine_mod.Engine, m)


def test_no_option_key():
    """The switch is a typed setter: az_set_option's body names no new key, and the rule's header states the property it rests on."""
    src = open(os.path.join(ROOT, "alphazero-rs_amd", "csrc", "az_engine.hip")).read()
    body = src[src.index("az_status az_set_option("):src.index("az_status az_get_stats(")]
    assert "search_stop" not in body and "stop" not in re.findall(r'is\("(\w+)"\)', body)
    rule = open(os.path.join(ROOT, "alphazero-rs_amd", "csrc", "az_stop.h")).read()
    assert "raises exactly one root" in rule and "DIFFER" in rule and "__global__" not in rule
    host = open(os.path.join(ROOT, "include", "az_host.hpp")).read()
    assert "inline void set_search_stop(" in host and "search_stop_stats(" in host
