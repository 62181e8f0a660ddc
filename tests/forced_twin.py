"""ctypes wrapper of the forced-playouts twin (tests/cpp/forced_twin.cpp): the oracle's search and episode loop with forced playouts at
the root and policy target pruning ("forced_playouts_k_e6" / "policy_prune", include/az_engine.h) restated around it, and the g++ build
of csrc/az_forced.h.  TEST INFRASTRUCTURE ONLY.

The library is compiled once per process into a temporary directory (g++ -O2 -ffp-contract=off, as the playout-cap twin)."""
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
# the twin's counters (forced_twin.cpp): root selections compared, those whose winner had u = +inf, those of them made while earlier
# simulations of the step were in flight, moves compared, moves whose pruned counts differ from the raw ones, children pruned from
# >= 2 visits to 0 by the single-playout rule, root-child visits, visits pruned
COUNTERS = ("root_sel", "root_forced", "root_forced_inflight", "moves", "moves_pruned", "to_zero", "visits", "visits_pruned")

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="forced_twin_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libforced_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"),
                               "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "forced_twin.cpp"), "-o", so])
        L = C.CDLL(so)
        u64, i64, i32, vp, f32 = C.c_uint64, C.c_int64, C.c_int32, C.c_void_p, C.c_float
        L.twin_forced_counters.restype = i32; L.twin_forced_counters.argtypes = []
        L.twin_forced_eval.restype = None; L.twin_forced_eval.argtypes = [i64, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp]
        L.twin_forced_puct.restype = None; L.twin_forced_puct.argtypes = [i64, vp, vp, vp, vp, f32, vp]
        L.twin_forced_tree_new.restype = vp; L.twin_forced_tree_new.argtypes = [i32, u64, u64, u64, u64, i32, i32, u64]
        L.twin_forced_tree_free.restype = None; L.twin_forced_tree_free.argtypes = [vp]
        L.twin_forced_tree_get_action_prob.restype = i32
        L.twin_forced_tree_get_action_prob.argtypes = [vp, u64, u64, f32, u64, u64, i64, i64, i64, i32, vp, vp, vp, vp]
        L.twin_forced_selfplay.restype = i64
        L.twin_forced_selfplay.argtypes = [i64, u64, u64, u64, i64, u64, i32, u64, u64, u64, i32, u64, i32, i32, i64, i64, i64, i32,
                                           vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        assert L.twin_forced_counters() == len(COUNTERS)
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def e6(x):
    return int(round(float(x) * 1e6))


def default_reserve(sims):
    return 8 + 42 * (7 * sims + 8)


def counters(arr):
    return {k: int(v) for k, v in zip(COUNTERS, arr)}


def add_counters(a, b):
    return {k: a.get(k, 0) + b[k] for k in COUNTERS}


# ---- the g++ build of csrc/az_forced.h, element by element --------------------------------------------------------------------------------
def host_eval(k_e6, p, S, n, q, n_root, cpuct, u_star):
    """nf [N] f32, forced [N] bool, m [N] u32 (the pruned count of a slot with n visits) and sq [N] f32 = sqrt(N_root + 1e-6)."""
    k_e6 = np.ascontiguousarray(k_e6, np.int64); p = np.ascontiguousarray(p, np.float32); S = np.ascontiguousarray(S, np.uint32)
    n = np.ascontiguousarray(n, np.uint32); q = np.ascontiguousarray(q, np.float32); n_root = np.ascontiguousarray(n_root, np.uint32)
    u_star = np.ascontiguousarray(u_star, np.float32)
    N = len(p)
    nf, forced, m, sq = np.zeros(N, np.float32), np.zeros(N, np.uint8), np.zeros(N, np.uint32), np.zeros(N, np.float32)
    lib().twin_forced_eval(N, _p(k_e6), _p(p), _p(S), _p(n), _p(q), _p(n_root), float(cpuct), _p(u_star), _p(nf), _p(forced), _p(m), _p(sq))
    return nf, forced.astype(bool), m, sq


def host_puct(q, n, p, n_root, cpuct):
    q = np.ascontiguousarray(q, np.float32); n = np.ascontiguousarray(n, np.uint32); p = np.ascontiguousarray(p, np.float32)
    n_root = np.ascontiguousarray(n_root, np.uint32)
    out = np.zeros(len(q), np.float32)
    lib().twin_forced_puct(len(q), _p(q), _p(n), _p(p), _p(n_root), float(cpuct), _p(out))
    return out


# ---- the predicates restated with numpy f32 (every operation rounds once to f32; np.sqrt of an f32 is correctly rounded) ------------------
def nf_py(k_e6, p, S):
    f = np.float32
    return np.sqrt(f(f(f(k_e6 / 1e6) * f(p)) * f(S)))


def sq_py(n_root):
    return np.sqrt(np.float32(np.float32(n_root) + np.float32(1e-6)))


def puct_py(q, n, p, sq, cpuct):
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):               # n = 65535: the u16 denominator wraps to 0, as in the reference
        return f(f(q) + f(f(f(f(cpuct) * f(p)) * f(sq)) / f((n + 1) & 0xFFFF)))


def prune_py(k_e6, p, S, n, q, sq, cpuct, u_star):
    f = np.float32
    fj = int(nf_py(k_e6, p, S))
    lo = n - fj if n > fj else 0
    c = f(f(f(cpuct) * f(p)) * f(sq))
    m = n
    while m > lo and f(f(q) + f(c / f(m))) < f(u_star):
        m -= 1
    if m != n and m == 1:
        m = 0
    return m


# ---- one AsyncMcts with the feature ---------------------------------------------------------------------------------------------------------
class Tree:
    def __init__(self, sims, net_kind=NET_HASH, salt=0, cpuct=1, max_depth=1000, reserve=None, threads=1, game_kind=GAME_BITS):
        self.h = lib().twin_forced_tree_new(game_kind, reserve or default_reserve(sims), sims, threads, max_depth, cpuct, net_kind, salt)
        assert self.h
        self.ctr = np.zeros(len(COUNTERS), np.uint64)

    def get_action_prob(self, state, temp, seed, game_id, k=0.0, prune=0, eps=0.0, alpha=1.0):
        pi, counts, q = np.zeros(7, np.float32), np.zeros(7, np.uint16), np.zeros(7, np.float32)
        rc = lib().twin_forced_tree_get_action_prob(self.h, int(state[0]), int(state[1]), float(temp), seed, game_id, e6(eps), e6(alpha), e6(k),
                                                    int(prune), _p(pi), _p(counts), _p(q), _p(self.ctr))
        if rc != 0:
            raise RuntimeError("twin get_action_prob failed")
        return pi, counts, q

    def close(self):
        if self.h:
            lib().twin_forced_tree_free(self.h)
            self.h = None

    __del__ = close


def selfplay(n_games, sims, k=0.0, prune=0, cap_sims=0, full_e6=250000, net_kind=NET_STUB, salt=0, seed=0, first_game_id=0, temp_threshold=15,
             cpuct=1, max_depth=1000, reserve=None, game_kind=GAME_BITS, replay=None, sim_threads=1, eps=0.0, alpha=1.0):
    """Coach::execute_episode x n_games with forced playouts (k) and pruning on the full moves -- every move when cap_sims == 0.  The fields
    of playout_cap_twin.selfplay plus `ctr`, the twin's counters by name."""
    cap = n_games * 84
    boards, pis, zs = np.zeros((cap, 2, 6, 7), np.float32), np.zeros((cap, 7), np.float32), np.zeros(cap, np.float32)
    game_len, moves, bad = np.zeros(n_games, np.int32), np.zeros((n_games, 42), np.uint8), np.zeros(n_games, np.int32)
    masks, sims_out, ctr = np.zeros(n_games, np.uint64), np.zeros(2, np.uint64), np.zeros(len(COUNTERS), np.uint64)
    ro = rs = rp = rv = None
    if replay is not None:
        ro = np.ascontiguousarray(replay[0], np.int64)
        rs = None if replay[1] is None else np.ascontiguousarray(replay[1], np.uint64)
        rp, rv = np.ascontiguousarray(replay[2], np.float32), np.ascontiguousarray(replay[3], np.float32)
    n = lib().twin_forced_selfplay(n_games, first_game_id, sims, cap_sims, full_e6, temp_threshold, cpuct, max_depth, reserve or default_reserve(sims),
                                   seed, net_kind, salt, game_kind, sim_threads, e6(eps), e6(alpha), e6(k), int(prune), _p(boards), _p(pis),
                                   _p(zs), cap, _p(game_len), _p(moves), _p(masks), _p(sims_out), _p(ctr), _p(ro), _p(rs), _p(rp), _p(rv), _p(bad))
    if n < 0:
        raise RuntimeError("twin forced selfplay failed")
    return {"count": int(n), "game_len": game_len, "moves": moves, "replay_bad": bad, "boards": boards[:n], "pis": pis[:n], "zs": zs[:n],
            "full_masks": masks, "sims": int(sims_out[0]), "budgets": int(sims_out[1]), "ctr": counters(ctr)}
