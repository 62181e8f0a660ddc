"""az_reanalyse without a GPU (include/az_reanalyse.h, csrc/az_reanalyse.h): the library exports the entry outside include/az_engine.h and
engine.EXPORTS, the ctypes struct has the header's size, the position rule as g++ builds it (tests/cpp/reanalyse_twin.cpp) agrees with a
numpy restatement written here on hand-made positions, and the Coaches' rule -- which history entries, which game ids -- is one rule in
csrc/az_reanalyse.h, include/az_host.hpp and alphazero-rs_amd."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, FEATURE, FLOATING, COUNTS, DECIDED = 2, 4, 16, 32, 64
TEXT = {0: "-", STATE: "a state with overlapping stones or bits outside the 7x6 board",
        FEATURE: "a boards feature that is not 0 or 1, or a cell set in both planes", FLOATING: "a stone above an empty cell",
        COUNTS: "stone counts that no game reaches (theirs - mine must be 0 or 1)", DECIDED: "a position that is already decided or full"}


def bit(c, r):
    return 1 << (c * 7 + r)


def play(moves):
    """(mine, theirs) after the column sequence `moves` from the empty board, the side to move as `mine`."""
    mine, theirs, height = 0, 0, [0] * 7
    for c in moves:
        mine, theirs = theirs, mine | bit(c, height[c])
        height[c] += 1
    return mine, theirs


def rule_np(mine, theirs):
    """The verdict bits, cell by cell: no shifts of whole boards, no popcount tricks."""
    cells = np.zeros((2, 7, 8), np.int64)          # [side][column][row]; rows 6 and 7 and column bits beyond are outside the board
    outside = False
    for b in range(64):
        for side, word in enumerate((mine, theirs)):
            if (word >> b) & 1:
                c, r = divmod(b, 7)
                if c >= 7 or r >= 6:
                    outside = True
                else:
                    cells[side, c, r] = 1
    if outside or (mine & theirs):
        return STATE
    bad = 0
    occ = cells[0] + cells[1]
    for c in range(7):
        for r in range(1, 6):
            if occ[c, r] and not occ[c, r - 1]:
                bad |= FLOATING
    if int(cells[1].sum()) - int(cells[0].sum()) not in (0, 1):
        bad |= COUNTS
    four = False
    for side in range(2):
        g = cells[side]
        for c in range(7):
            for r in range(6):
                for dc, dr in ((1, 0), (0, 1), (1, 1), (1, -1)):
                    ok = all(0 <= c + k * dc < 7 and 0 <= r + k * dr < 6 and g[c + k * dc, r + k * dr] for k in range(4))
                    four = four or ok
    if four or int(occ[:, :6].sum()) == 42:
        bad |= DECIDED
    return bad


FULL_DRAW = [0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0, 2, 3, 2, 3, 2, 3, 3, 2, 3, 2, 3, 2, 4, 5, 4, 5, 4, 5, 5, 4, 5, 4, 5, 4, 6, 6, 6, 6, 6, 6]

POSITIONS = {
    "empty": ((0, 0), 0),
    "one_stone": (play([3]), 0),
    "mid_game": (play([3, 3, 4, 2, 4, 4, 0]), 0),
    "floating": ((0, bit(2, 1)), FLOATING),
    "floating_high": ((bit(5, 0), bit(5, 2) | bit(0, 0)), FLOATING),
    "counts_off_by_two": ((0, bit(0, 0) | bit(1, 0)), COUNTS),
    "mover_ahead": ((bit(0, 0), 0), COUNTS),
    "decided_row": (play([0, 0, 1, 1, 2, 2, 3]), DECIDED),
    "decided_column": (play([0, 1, 0, 1, 0, 1, 0]), DECIDED),
    "decided_diagonal": (play([0, 1, 1, 2, 3, 2, 2, 3, 3, 6, 3]), DECIDED),
    "full": (play(FULL_DRAW), DECIDED),
    "outside_row_6": ((0, bit(4, 6)), STATE),
    "outside_bit_63": ((1 << 63, 0), STATE),
    "overlap": ((bit(3, 0), bit(3, 0)), STATE),
    "floating_and_counts": ((0, bit(2, 1) | bit(3, 3)), FLOATING | COUNTS),
}


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    exe = os.path.join(tmp_path_factory.mktemp("reanalyse"), "reanalyse_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "reanalyse_twin.cpp"), "-o", exe])
    return exe


def first_text(bits):
    for b in (FEATURE, STATE, FLOATING, COUNTS, DECIDED):
        if bits & b:
            return TEXT[b]
    return TEXT[0]


def test_full_board_fixture_is_a_draw():
    mine, theirs = play(FULL_DRAW)
    assert bin(mine | theirs).count("1") == 42 and rule_np(mine, theirs) == DECIDED
    # ... for being full, not for a line: one stone fewer is an open position
    assert rule_np(*play(FULL_DRAW[:-1])) == 0


def test_position_rule_against_numpy(twin):
    names = sorted(POSITIONS)
    text = "".join("%x %x\n" % POSITIONS[n][0] for n in names)
    out = subprocess.run([twin, "positions"], input=text, check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()
    assert len(out) == len(names)
    for n, line in zip(names, out):
        bits, why = line.split(" ", 1)
        (mine, theirs), want = POSITIONS[n]
        assert int(bits) == want == rule_np(mine, theirs), (n, bits, want, rule_np(mine, theirs))
        assert why == first_text(want), n


def test_position_rule_on_random_walks(twin):
    """Every position of random games is playable until the game ends; the rule agrees with numpy on each and on one-bit damage."""
    rng = np.random.default_rng(5)
    cases = []
    for _ in range(12):
        moves, height = [], [0] * 7
        while True:
            mine, theirs = play(moves)
            cases.append((mine, theirs))
            cases.append((mine ^ (1 << int(rng.integers(0, 49))), theirs))
            if rule_np(mine, theirs) & DECIDED:
                break
            c = int(rng.choice([c for c in range(7) if height[c] < 6]))
            moves.append(c)
            height[c] += 1
    text = "".join("%x %x\n" % c for c in cases)
    out = subprocess.run([twin, "positions"], input=text, check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()
    assert len(out) == len(cases) > 100
    seen = set()
    for (mine, theirs), line in zip(cases, out):
        got = int(line.split(" ", 1)[0])
        assert got == rule_np(mine, theirs), (hex(mine), hex(theirs), got)
        seen.add(got)
    assert {0, DECIDED, FLOATING} <= seen


def test_planes_route(twin):
    """The boards route rebuilds the state (az_samples.h) and then applies the same rule; a bad feature carries its own verdict alone."""
    import mirror_twin
    names = ["mid_game", "floating", "decided_row", "counts_off_by_two"]
    states = np.array([POSITIONS[n][0] for n in names], np.uint64)
    boards = mirror_twin.states_to_boards(states).reshape(len(names), 84).copy()
    extra = boards[0].copy()
    extra[5 * 7 + 6] = 0.5
    rows = list(boards) + [extra]
    text = "\n".join(" ".join("%g" % x for x in r) for r in rows) + "\n"
    out = subprocess.run([twin, "planes"], input=text, check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()
    assert len(out) == len(rows)
    for n, line in zip(names, out):
        b, m, t = line.split()
        assert int(b) == POSITIONS[n][1] and (int(m, 16), int(t, 16)) == POSITIONS[n][0], n
    assert int(out[-1].split()[0]) == FEATURE


def test_coach_rule_is_one_rule(twin, engine_mod):
    from alphazero_rs_amd import coach
    out = subprocess.run([twin, "rule"], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()
    ids = set()
    rows = 0
    for line in out:
        w = line.split()
        if w[0] == "id":
            it, h, a, b = int(w[1]), int(w[2]), int(w[3], 16), int(w[4], 16)
            assert a == b == engine_mod.reanalyse_first_game_id(it, h) == coach.reanalyse_first_game_id(it, h)
            ids.add(a)
            rows += 1
        elif w[0] == "max":
            assert int(w[1]) == 1 << 24 and int(w[3]) == 8192 and int(w[5], 16) == int(w[6], 16) == engine_mod.REANALYSE_ID_BASE == 1 << 62
        else:
            it, n, a, b = (int(x) for x in w)
            assert a == b == coach.reanalyse_entries(n) == max(n - 1, 0)
    assert rows == 4 * (0 + 0 + 1 + 2 + 3 + 4) and len(ids) == 4 * 4   # every (iteration, entry) pair has a block of ids of its own
    blocks = sorted(ids)
    assert all(y - x >= 1 << 32 for x, y in zip(blocks, blocks[1:])) and blocks[0] >= 1 << 62


def test_library_exports_the_entry_outside_the_main_header(engine_mod):
    lib = ctypes.CDLL(engine_mod.LIB_PATH)
    assert hasattr(lib, "az_reanalyse")
    assert engine_mod.EXT_EXPORTS == ["az_reanalyse"]
    assert "az_reanalyse" not in engine_mod.EXPORTS
    assert "az_reanalyse" not in open(os.path.join(ROOT, "include", "az_engine.h")).read()
    hdr = open(os.path.join(ROOT, "include", "az_reanalyse.h")).read()
    assert '#include "az_engine.h"' in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(az_[a-z_0-9]+)\s*\(", code))) == engine_mod.EXT_EXPORTS
    # no new option key came with it: the entry takes everything in its params struct
    src = open(os.path.join(ROOT, "alphazero-rs_amd", "csrc", "az_engine.hip")).read()
    body = src[src.index("az_status az_set_option("):src.index("\naz_status az_get_stats(")]
    assert "reanalyse" not in body


def test_struct_layout_matches_the_header(engine_mod, tmp_path):
    """sizeof and every field offset of az_reanalyse_params, as g++ lays the header's struct out."""
    fields = [n for n, _ in engine_mod.az_reanalyse_params._fields_]
    src = os.path.join(tmp_path, "layout.c")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "az_reanalyse.h"\nint main(void) {\n')
        f.write('    printf("%zu\\n", sizeof(az_reanalyse_params));\n')
        for n in fields:
            f.write('    printf("%%zu\\n", offsetof(az_reanalyse_params, %s));\n' % n)
        f.write("    return 0;\n}\n")
    exe = os.path.join(tmp_path, "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(engine_mod.az_reanalyse_params) == 56
    assert out[1:] == [getattr(engine_mod.az_reanalyse_params, n).offset for n in fields]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "az_reanalyse.h")).read(), flags=re.S)
    body = re.search(r"typedef struct az_reanalyse_params \{(.*?)\}", hdr, flags=re.S).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == fields
