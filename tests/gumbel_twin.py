"""ctypes wrapper of the Gumbel twin (tests/cpp/gumbel_twin.cpp): the oracle's search and episode loop with Gumbel root search and
sequential halving restated around them ("gumbel_m" of include/az_engine.h, alone and with root noise / a playout cap), and the g++ build
of csrc/az_gumbel.h.  TEST INFRASTRUCTURE ONLY.

The library is compiled once per process into a temporary directory (g++ -O2 -ffp-contract=off, the flags the header states)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_STUB, NET_HASH, NET_REPLAY = 0, 1, 2
GAME_BITS, GAME_CONNECT3 = 0, 2
M64 = (1 << 64) - 1
RNG_GUMBEL = 8
# the twin's counters (gumbel_twin.cpp): root selections, those whose winner is not the PUCT winner of the same state, Gumbel moves, moves
# whose selected action is not the most visited one, moves on a reused root with a non-zero baseline, root selections that found no
# considered slot (must be 0), moves whose final visits are not the prescribed schedule (must be 0), moves with every variate 0 (temp 0),
# moves in which a placeholder slot of the root became a link to a node an earlier move built (its baseline is then that node's count)
COUNTERS = ("root_sel", "root_not_puct", "moves", "moves_not_most_visited", "moves_reused", "no_considered", "bad_schedule", "moves_g_zero",
            "moves_relinked")

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="gumbel_twin_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libgumbel_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cpp", "gumbel_twin.cpp"), "-o", so])
        L = C.CDLL(so)
        u64, i64, i32, u32, f32, vp = C.c_uint64, C.c_int64, C.c_int32, C.c_uint32, C.c_float, C.c_void_p
        L.gtwin_counters.restype = i32; L.gtwin_counters.argtypes = []
        L.gtwin_considered.restype = None; L.gtwin_considered.argtypes = [u32, u32, i64, vp]
        L.gtwin_prescribed_d.restype = None; L.gtwin_prescribed_d.argtypes = [u32, u32, u32, vp]
        L.gtwin_uniform.restype = None; L.gtwin_uniform.argtypes = [i64, vp, vp]
        L.gtwin_of_uniform.restype = None; L.gtwin_of_uniform.argtypes = [i64, vp, vp]
        L.gtwin_logit.restype = None; L.gtwin_logit.argtypes = [i64, vp, vp]
        L.gtwin_values.restype = None; L.gtwin_values.argtypes = [i64, u64, vp, vp, i32, vp]
        L.gtwin_root.restype = None; L.gtwin_root.argtypes = [u32, vp, vp, vp, vp, vp, u32, u32, i64, i64, vp, vp, vp]
        L.gtwin_tree_new.restype = vp; L.gtwin_tree_new.argtypes = [i32, u64, u64, u64, u64, i32, i32, u64]
        L.gtwin_tree_free.restype = None; L.gtwin_tree_free.argtypes = [vp]
        L.gtwin_tree_get_action_prob.restype = i32
        L.gtwin_tree_get_action_prob.argtypes = [vp, u64, u64, f32, u64, u64, i32, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp]
        L.gtwin_selfplay.restype = i64
        L.gtwin_selfplay.argtypes = [i64, u64, u64, u64, i64, u64, i32, u64, u64, u64, i32, u64, i32, i32, i64, i64, i64, i64,
                                     vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        assert L.gtwin_counters() == len(COUNTERS)
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def e6(x):
    """The option value of a real c_visit / c_scale / eps (what Engine.set_gumbel sends)."""
    return int(round(float(x) * 1e6))


def default_reserve(sims):
    return 8 + 42 * (7 * sims + 8)


def counters(arr):
    return {k: int(v) for k, v in zip(COUNTERS, arr)}


def add_counters(a, b):
    return {k: a.get(k, 0) + b[k] for k in COUNTERS}


# ---- the g++ build of csrc/az_gumbel.h ---------------------------------------------------------------------------------------------------
def considered(m_eff, n, count=None):
    out = np.zeros(n if count is None else count, np.uint32)
    lib().gtwin_considered(m_eff, n, len(out), _p(out))
    return out


def prescribed_d(m_eff, n, nchild):
    out = np.zeros(nchild, np.uint32)
    lib().gtwin_prescribed_d(m_eff, n, nchild, _p(out))
    return out


def uniform(r):
    r = np.ascontiguousarray(r, np.uint64)
    out = np.empty(r.shape, np.float32)
    lib().gtwin_uniform(r.size, _p(r), _p(out))
    return out


def of_uniform(u):
    u = np.ascontiguousarray(u, np.float32)
    out = np.empty_like(u)
    lib().gtwin_of_uniform(u.size, _p(u), _p(out))
    return out


def logit(p):
    p = np.ascontiguousarray(p, np.float32)
    out = np.empty_like(p)
    lib().gtwin_logit(p.size, _p(p), _p(out))
    return out


def values(states, game_ids, seed=0, temp_is_zero=False):
    """Host build of the variates: g [n,7] for root states [n,2] on the streams (seed, game_ids[i], stones)."""
    s = np.ascontiguousarray(states, np.uint64).reshape(-1, 2)
    g = np.ascontiguousarray(game_ids, np.uint64).reshape(-1)
    assert len(g) == len(s)
    out = np.empty((len(s), 7), np.float32)
    lib().gtwin_values(len(s), seed, _p(g), _p(s), 1 if temp_is_zero else 0, _p(out))
    return out


def root(p, q, g, n, base, m, budget, c_visit=50.0, c_scale=1.0):
    """One root through the g++ build: (slot the next simulation goes to, whether a considered slot existed, selected slot of the result,
    sigma [nchild], pi by slot [nchild])."""
    p = np.ascontiguousarray(p, np.float32); q = np.ascontiguousarray(q, np.float32); g = np.ascontiguousarray(g, np.float32)
    n = np.ascontiguousarray(n, np.uint32); base = np.ascontiguousarray(base, np.uint32)
    k = len(p)
    sel, sigma, pi = np.zeros(3, np.uint32), np.zeros(7, np.float32), np.zeros(7, np.float32)
    lib().gtwin_root(k, _p(p), _p(q), _p(g), _p(n), _p(base), m, budget, e6(c_visit), e6(c_scale), _p(sel), _p(sigma), _p(pi))
    return int(sel[0]), bool(sel[1]), int(sel[2]), sigma[:k], pi[:k]


# ---- mix64 / rng_draw of csrc/az_common.h ---------------------------------------------------------------------------------------------------
def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rng_draw(seed, game_id, ply, purpose):
    return mix64(mix64(mix64(mix64(seed) ^ game_id) ^ ply) ^ purpose)


# ---- one AsyncMcts whose get_action_prob is a Gumbel move ------------------------------------------------------------------------------------
class Tree:
    """One AsyncMcts of the oracle searched by the Gumbel rule (m > 0; m = 0: the oracle's own get_action_prob).  `ctr` accumulates the
    twin's counters over the calls."""

    def __init__(self, sims, net_kind=NET_STUB, salt=0, cpuct=1, max_depth=1000, reserve=None, model_id=0, game_kind=GAME_BITS):
        self._h = lib().gtwin_tree_new(game_kind, reserve or default_reserve(sims), sims, max_depth, model_id, cpuct, net_kind, salt)
        if not self._h:
            raise RuntimeError("gtwin_tree_new failed")
        self.ctr = np.zeros(len(COUNTERS), np.uint64)

    def get_action_prob(self, mine, theirs, temp, seed=0, game_id=0, m=4, c_visit=50.0, c_scale=1.0, eps=0.0, alpha=1.0):
        """-> pi [7], counts [7], q [7], selected action, d [7] (visits of this call by slot)."""
        pi, counts, q = np.zeros(7, np.float32), np.zeros(7, np.uint16), np.zeros(7, np.float32)
        sel, d = np.zeros(1, np.int32), np.zeros(7, np.uint32)
        rc = lib().gtwin_tree_get_action_prob(self._h, int(mine), int(theirs), temp, seed, game_id, m, e6(c_visit), e6(c_scale), e6(eps), e6(alpha),
                                              _p(pi), _p(counts), _p(q), _p(sel), _p(d), _p(self.ctr))
        if rc != 0:
            raise RuntimeError("twin get_action_prob failed (terminal root or reserve exhausted)")
        return pi, counts, q, int(sel[0]), d

    def close(self):
        if self._h:
            lib().gtwin_tree_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def selfplay(n_games, sims, m, c_visit=50.0, c_scale=1.0, net_kind=NET_STUB, salt=0, seed=0, first_game_id=0, temp_threshold=15, cpuct=1,
             max_depth=1000, reserve=None, game_kind=GAME_BITS, replay=None, eps=0.0, alpha=1.0, cap_sims=0, full_e6=250000):
    """Coach::execute_episode x n_games with Gumbel moves.  Full moves (every move when cap_sims == 0) are Gumbel moves of `sims` simulations,
    noisy when eps > 0, and are recorded with the improved policy; fast moves search `cap_sims` by PUCT and are only played.  The fields of
    oracle_py.selfplay plus full_masks [n_games], sims (the oracle's simulation counter), budgets and ctr (the twin's counters by name)."""
    cap = n_games * 84
    boards, pis, zs = np.zeros((cap, 2, 6, 7), np.float32), np.zeros((cap, 7), np.float32), np.zeros(cap, np.float32)
    game_len, moves, bad = np.zeros(n_games, np.int32), np.zeros((n_games, 42), np.uint8), np.zeros(n_games, np.int32)
    masks, sims_out, ctr = np.zeros(n_games, np.uint64), np.zeros(2, np.uint64), np.zeros(len(COUNTERS), np.uint64)
    ro = rs = rp = rv = None
    if replay is not None:
        ro = np.ascontiguousarray(replay[0], np.int64)
        rs = None if replay[1] is None else np.ascontiguousarray(replay[1], np.uint64)
        rp, rv = np.ascontiguousarray(replay[2], np.float32), np.ascontiguousarray(replay[3], np.float32)
    n = lib().gtwin_selfplay(n_games, first_game_id, sims, cap_sims, full_e6, temp_threshold, cpuct, max_depth, reserve or default_reserve(sims),
                             seed, net_kind, salt, game_kind, m, e6(c_visit), e6(c_scale), e6(eps), e6(alpha), _p(boards), _p(pis), _p(zs),
                             cap, _p(game_len), _p(moves), _p(masks), _p(sims_out), _p(ctr), _p(ro), _p(rs), _p(rp), _p(rv), _p(bad))
    if n < 0:
        raise RuntimeError("twin selfplay failed")
    return {"count": int(n), "game_len": game_len, "moves": moves, "replay_bad": bad, "boards": boards[:n], "pis": pis[:n], "zs": zs[:n],
            "full_masks": masks, "sims": int(sims_out[0]), "budgets": int(sims_out[1]), "ctr": counters(ctr)}
