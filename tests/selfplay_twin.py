"""ctypes wrapper of the self-play twin (tests/cpp/selfplay_twin.cpp): the oracle's search and episode loop with the engine's self-play
options restated around them -- Dirichlet root noise, playout cap randomization, forced playouts at the root and policy target pruning
(include/az_engine.h) -- and the g++ builds of csrc/az_noise.h, az_playout.h and az_forced.h.  TEST INFRASTRUCTURE ONLY.

The library is compiled once per process into a temporary directory (g++ -O2 -ffp-contract=off, the flags the headers state)."""
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
RNG_PLAYOUT_CAP = 6
# the twin's counters (selfplay_twin.cpp): root selections compared, those whose winner had u = +inf, those of them made while earlier
# simulations of the step were in flight, moves compared, moves whose pruned counts differ from the raw ones, children pruned from
# >= 2 visits to 0 by the single-playout rule, root-child visits, visits pruned
COUNTERS = ("root_sel", "root_forced", "root_forced_inflight", "moves", "moves_pruned", "to_zero", "visits", "visits_pruned")

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="selfplay_twin_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libselfplay_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cpp", "selfplay_twin.cpp"), "-o", so])
        L = C.CDLL(so)
        u64, i64, i32, f32, vp = C.c_uint64, C.c_int64, C.c_int32, C.c_float, C.c_void_p
        L.twin_noise_eta.restype = None; L.twin_noise_eta.argtypes = [i64, u64, vp, vp, i64, vp]
        L.twin_noise_log2.restype = None; L.twin_noise_log2.argtypes = [i64, vp, vp]
        L.twin_noise_exp2.restype = None; L.twin_noise_exp2.argtypes = [i64, vp, vp]
        L.twin_playout_full.restype = None; L.twin_playout_full.argtypes = [i64, u64, vp, vp, i64, vp]
        L.twin_playout_thresh24.restype = C.c_uint32; L.twin_playout_thresh24.argtypes = [i64]
        L.twin_forced_counters.restype = i32; L.twin_forced_counters.argtypes = []
        L.twin_forced_eval.restype = None; L.twin_forced_eval.argtypes = [i64, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp]
        L.twin_forced_puct.restype = None; L.twin_forced_puct.argtypes = [i64, vp, vp, vp, vp, f32, vp]
        L.twin_tree_new.restype = vp; L.twin_tree_new.argtypes = [i32, u64, u64, u64, u64, u64, i32, i32, u64]
        L.twin_tree_free.restype = None; L.twin_tree_free.argtypes = [vp]
        L.twin_tree_get_action_prob.restype = i32
        L.twin_tree_get_action_prob.argtypes = [vp, u64, u64, f32, u64, u64, i64, i64, i64, i32, vp, vp, vp, vp]
        L.twin_tree_root_priors.restype = i32; L.twin_tree_root_priors.argtypes = [vp, u64, u64, vp]
        L.twin_tree_set_replay.restype = None; L.twin_tree_set_replay.argtypes = [vp, vp, vp, vp, u64]
        L.twin_tree_replay_bad.restype = i32; L.twin_tree_replay_bad.argtypes = [vp]
        L.twin_selfplay.restype = i64
        L.twin_selfplay.argtypes = [i64, u64, u64, u64, i64, u64, i32, u64, u64, u64, i32, u64, i32, i32, i64, i64, i64, i32,
                                    vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        assert L.twin_forced_counters() == len(COUNTERS)
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def e6(x):
    """The option value of a real eps / alpha / k (what Engine.set_root_noise sends)."""
    return int(round(float(x) * 1e6))


def default_reserve(sims):
    return 8 + 42 * (7 * sims + 8)


def counters(arr):
    return {k: int(v) for k, v in zip(COUNTERS, arr)}


def add_counters(a, b):
    return {k: a.get(k, 0) + b[k] for k in COUNTERS}


# ---- the g++ build of csrc/az_noise.h --------------------------------------------------------------------------------------------------
def noise_eta(states, game_ids, alpha, seed=0):
    """Host build of the sampler: eta [n,7] for root states [n,2] on the streams (seed, game_ids[i], stones)."""
    s = np.ascontiguousarray(states, np.uint64).reshape(-1, 2)
    g = np.ascontiguousarray(game_ids, np.uint64).reshape(-1)
    assert len(g) == len(s)
    eta = np.empty((len(s), 7), np.float32)
    lib().twin_noise_eta(len(s), seed, _p(g), _p(s), e6(alpha), _p(eta))
    return eta


def noise_log2(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    lib().twin_noise_log2(x.size, _p(x), _p(out))
    return out


def noise_exp2(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    lib().twin_noise_exp2(x.size, _p(x), _p(out))
    return out


# ---- csrc/az_playout.h: the predicate restated in Python (mix64 / rng_draw of csrc/az_common.h) and its g++ build -------------------------
def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rng_draw(seed, game_id, ply, purpose):
    return mix64(mix64(mix64(mix64(seed) ^ game_id) ^ ply) ^ purpose)


def full_py(seed, game_id, ply, full_e6):
    return (rng_draw(seed, game_id, ply, RNG_PLAYOUT_CAP) >> 40) < (full_e6 << 24) // 1000000


def full_host(seed, game_ids, plies, full_e6):
    """The g++ build of csrc/az_playout.h: bool [n] for the moves (seed, game_ids[i], plies[i]) at P = full_e6."""
    g = np.ascontiguousarray(game_ids, np.uint64).reshape(-1)
    p = np.ascontiguousarray(plies, np.uint64).reshape(-1)
    assert len(g) == len(p)
    out = np.zeros(len(g), np.uint8)
    lib().twin_playout_full(len(g), seed, _p(g), _p(p), full_e6, _p(out))
    return out.astype(bool)


def popcount(masks):
    return int(sum(bin(int(m)).count("1") for m in np.asarray(masks).reshape(-1)))


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


# ---- one AsyncMcts under the options ----------------------------------------------------------------------------------------------------------
class Tree:
    """One AsyncMcts of the oracle whose get_action_prob is a full move: noise mixed in first (eps > 0), forced playouts at the root (k),
    pruned counts behind pi (prune).  `ctr` accumulates the twin's counters over the calls."""

    def __init__(self, sims, net_kind=NET_STUB, salt=0, cpuct=1, max_depth=1000, reserve=None, model_id=0, game_kind=GAME_BITS, threads=1):
        self._keep = None
        self._h = lib().twin_tree_new(game_kind, reserve or default_reserve(sims), sims, threads, max_depth, model_id, cpuct, net_kind, salt)
        if not self._h:
            raise RuntimeError("twin_tree_new failed")
        self.ctr = np.zeros(len(COUNTERS), np.uint64)

    def get_action_prob(self, mine, theirs, temp, seed=0, game_id=0, eps=0.0, alpha=1.0, k=0.0, prune=0):
        pi, counts, q = np.zeros(7, np.float32), np.zeros(7, np.uint16), np.zeros(7, np.float32)
        rc = lib().twin_tree_get_action_prob(self._h, int(mine), int(theirs), temp, seed, game_id, e6(eps), e6(alpha), e6(k), int(prune),
                                             _p(pi), _p(counts), _p(q), _p(self.ctr))
        if rc != 0:
            raise RuntimeError("twin get_action_prob failed (terminal root or reserve exhausted)")
        return pi, counts, q

    def root_priors(self, mine, theirs):
        """The stored prior p[0..7) of the node of state (mine, theirs)."""
        out = np.zeros(7, np.float32)
        if lib().twin_tree_root_priors(self._h, int(mine), int(theirs), _p(out)) != 0:
            raise RuntimeError("no such node, or it has no prior")
        return out

    def set_replay(self, states, pis, vs):
        self._keep = (np.ascontiguousarray(states, np.uint64), np.ascontiguousarray(pis, np.float32), np.ascontiguousarray(vs, np.float32))
        lib().twin_tree_set_replay(self._h, _p(self._keep[0]), _p(self._keep[1]), _p(self._keep[2]), len(self._keep[2]))

    def replay_bad(self):
        return bool(lib().twin_tree_replay_bad(self._h))

    def close(self):
        if self._h:
            lib().twin_tree_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def selfplay(n_games, sims, net_kind=NET_STUB, salt=0, seed=0, first_game_id=0, temp_threshold=15, cpuct=1, max_depth=1000, reserve=None,
             game_kind=GAME_BITS, replay=None, sim_threads=1, eps=0.0, alpha=1.0, cap_sims=0, full_e6=250000, k=0.0, prune=0):
    """Coach::execute_episode x n_games under the options.  Full moves (every move when cap_sims == 0) search `sims` simulations, noisy when
    eps > 0, with forced playouts (k) and pruning, and are recorded; fast moves search `cap_sims` and are only played.  The fields of
    oracle_py.selfplay plus full_masks [n_games] (bit ply = a full move), sims (the oracle's simulation counter), budgets (the sum of the
    moves' budgets) and ctr (the twin's counters by name)."""
    cap = n_games * 84
    boards, pis, zs = np.zeros((cap, 2, 6, 7), np.float32), np.zeros((cap, 7), np.float32), np.zeros(cap, np.float32)
    game_len, moves, bad = np.zeros(n_games, np.int32), np.zeros((n_games, 42), np.uint8), np.zeros(n_games, np.int32)
    masks, sims_out, ctr = np.zeros(n_games, np.uint64), np.zeros(2, np.uint64), np.zeros(len(COUNTERS), np.uint64)
    ro = rs = rp = rv = None
    if replay is not None:
        ro = np.ascontiguousarray(replay[0], np.int64)
        rs = None if replay[1] is None else np.ascontiguousarray(replay[1], np.uint64)
        rp, rv = np.ascontiguousarray(replay[2], np.float32), np.ascontiguousarray(replay[3], np.float32)
    n = lib().twin_selfplay(n_games, first_game_id, sims, cap_sims, full_e6, temp_threshold, cpuct, max_depth, reserve or default_reserve(sims),
                            seed, net_kind, salt, game_kind, sim_threads, e6(eps), e6(alpha), e6(k), int(prune), _p(boards), _p(pis), _p(zs),
                            cap, _p(game_len), _p(moves), _p(masks), _p(sims_out), _p(ctr), _p(ro), _p(rs), _p(rp), _p(rv), _p(bad))
    if n < 0:
        raise RuntimeError("twin selfplay failed")
    return {"count": int(n), "game_len": game_len, "moves": moves, "replay_bad": bad, "boards": boards[:n], "pis": pis[:n], "zs": zs[:n],
            "full_masks": masks, "sims": int(sims_out[0]), "budgets": int(sims_out[1]), "ctr": counters(ctr)}
