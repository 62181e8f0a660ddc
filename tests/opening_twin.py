"""ctypes wrapper of the opening twin (tests/cpp/opening_twin.cpp): the g++ build of csrc/az_opening.h -- paired arena openings
("arena_opening_plies" / az_arena_set_opening_book, include/az_engine.h) -- over the oracle's rules, and a pure-Python restatement of the
same rule that shares no text with either.  TEST INFRASTRUCTURE ONLY.

The library is compiled once per process into a temporary directory (g++ -O2, as the other twins)."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "alphazero-rs_amd", "csrc", "az_opening.h")
MAX_PLIES = 12
RNG_OPENING = 7

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="opening_twin_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libopening_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "oracle"),
                               "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "opening_twin.cpp"), "-o", so])
        L = C.CDLL(so)
        u64, i64, i32, vp = C.c_uint64, C.c_int64, C.c_int32, C.c_void_p
        L.twin_opening_rng_word.restype = i32; L.twin_opening_rng_word.argtypes = []
        L.twin_opening_max_plies.restype = i32; L.twin_opening_max_plies.argtypes = []
        L.twin_opening_grow.restype = i32; L.twin_opening_grow.argtypes = [i32, u64, i64, vp, vp, i32, vp, vp, vp, vp]
        assert L.twin_opening_rng_word() == RNG_OPENING and L.twin_opening_max_plies() == MAX_PLIES
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def grow(game, seed, pairs, n, bases=None):
    """The openings of `pairs` (global pair indices) with n plies under game 0 / 1, grown from bases [len(pairs), 2] (None = the initial
    board): boards [N,2] u64, len [N] i32, moves [N,12] u8, fallbacks [N] i32 (used plies drawn from C1 because no ply was quiet)."""
    pairs = np.ascontiguousarray(pairs, np.uint64)
    N = len(pairs)
    bases = np.zeros((N, 2), np.uint64) if bases is None else np.ascontiguousarray(np.broadcast_to(np.asarray(bases, np.uint64), (N, 2)))
    boards, ln, moves, fb = np.zeros((N, 2), np.uint64), np.zeros(N, np.int32), np.zeros((N, MAX_PLIES), np.uint8), np.zeros(N, np.int32)
    if lib().twin_opening_grow(int(game), int(seed), N, _p(pairs), _p(bases), int(n), _p(boards), _p(ln), _p(moves), _p(fb)) != 0:
        raise ValueError("twin_opening_grow refused its arguments")
    return boards, ln, moves, fb


def arena_openings(game, seed, total, plies, first=0, n_games=None, book=None, start_board=None):
    """What az_arena starts games first .. first + n_games of a `total`-game arena from: game g belongs to pair p = g % (total // 2), whose base
    is book[p % len(book)], else start_board, else the initial board.  (boards, len, moves) as grow()."""
    half = total // 2
    g = np.arange(first, first + (2 * half - first if n_games is None else n_games), dtype=np.int64)
    pairs = g % half
    if book is not None and len(book):
        bases = np.asarray(book, np.uint64).reshape(-1, 2)[pairs % len(book)]
    else:
        bases = np.broadcast_to(np.asarray((0, 0) if start_board is None else start_board, np.uint64), (len(g), 2))
    return grow(game, seed, pairs, plies, bases)[:3]


# ---- the rule restated in pure Python: columns of 7 bits, bit col * 7 + row, row 0 at the bottom; state = (mover's stones, other's stones) ----
M64 = (1 << 64) - 1
_FULL = sum(0x3F << (7 * c) for c in range(7))


def _mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _draw(seed, pair, j):
    return _mix64(_mix64(_mix64(_mix64(seed) ^ pair) ^ j) ^ RNG_OPENING)


def _line(b, k):
    """b holds k stones in a row: vertically, horizontally or on a diagonal"""
    for d in (1, 7, 6, 8):
        m = b
        for i in range(1, k):
            m &= b >> (d * i)
        if m:
            return True
    return False


def _legal(s):
    occ = s[0] | s[1]
    return [c for c in range(7) if not occ & (1 << (7 * c + 5))]


def _play(s, c):
    occ = s[0] | s[1]
    row = bin((occ >> (7 * c)) & 0x3F).count("1")
    return (s[1], s[0] | (1 << (7 * c + row)))           # the other side is to move


def _ended(s, k):
    """0: goes on; 'won': the player who just moved (s[1]) has a line; 'lost' / 'draw'"""
    if _line(s[0], k):
        return "lost"
    if _line(s[1], k):
        return "won"
    return "draw" if (s[0] | s[1]) == _FULL else 0


def win_in_one(s, k):
    return any(_ended(_play(s, b), k) == "won" for b in _legal(s))


@functools.lru_cache(maxsize=None)
def _candidates(s, k):
    c1 = [a for a in _legal(s) if _ended(_play(s, a), k) == 0]
    c2 = [a for a in c1 if not win_in_one(_play(s, a), k)]
    return (tuple(c2), False) if c2 else (tuple(c1), True)


@functools.lru_cache(maxsize=None)
def _line_of_play(game, seed, pair, base):
    """every ply the rule plays onto base for j = 0 .. 11 (ply j does not depend on n): [(action, state behind it, drawn from C1)]"""
    k, s, out = (4, 3)[game], base, []
    for j in range(MAX_PLIES):
        c, fell_back = _candidates(s, k)
        if not c:
            break
        a = c[((_draw(seed, pair, j) >> 32) * len(c)) >> 32]
        s = _play(s, a)
        out.append((a, s, fell_back))
    return out


def opening_py(game, seed, pair, n, base=(0, 0)):
    """(board, len, moves, fallbacks) of the opening with n plies: the longest even prefix of the first n plies played"""
    line = _line_of_play(game, int(seed), int(pair), (int(base[0]), int(base[1])))[:n]
    ln = len(line) & ~1
    board = line[ln - 1][1] if ln else (int(base[0]), int(base[1]))
    return board, ln, [a for a, _, _ in line[:ln]], sum(1 for _, _, f in line[:ln] if f)
