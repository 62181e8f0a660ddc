"""ctypes wrapper of the root-noise twin (tests/cpp/noise_twin.cpp): the oracle's search and episode loop with the Dirichlet root
noise of include/az_engine.h restated around them, and the g++ build of csrc/az_noise.h.  TEST INFRASTRUCTURE ONLY.

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

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="noise_twin_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libnoise_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cpp", "noise_twin.cpp"), "-o", so])
        L = C.CDLL(so)
        u64, i64, i32, f32, vp = C.c_uint64, C.c_int64, C.c_int32, C.c_float, C.c_void_p
        L.twin_noise_eta.restype = None; L.twin_noise_eta.argtypes = [i64, u64, vp, vp, i64, vp]
        L.twin_noise_log2.restype = None; L.twin_noise_log2.argtypes = [i64, vp, vp]
        L.twin_noise_exp2.restype = None; L.twin_noise_exp2.argtypes = [i64, vp, vp]
        L.twin_tree_new.restype = vp; L.twin_tree_new.argtypes = [i32, u64, u64, u64, u64, u64, i32, i32, u64]
        L.twin_tree_free.restype = None; L.twin_tree_free.argtypes = [vp]
        L.twin_tree_get_action_prob.restype = i32
        L.twin_tree_get_action_prob.argtypes = [vp, u64, u64, f32, u64, u64, i64, i64, vp, vp, vp]
        L.twin_tree_root_priors.restype = i32; L.twin_tree_root_priors.argtypes = [vp, u64, u64, vp]
        L.twin_tree_set_replay.restype = None; L.twin_tree_set_replay.argtypes = [vp, vp, vp, vp, u64]
        L.twin_tree_replay_bad.restype = i32; L.twin_tree_replay_bad.argtypes = [vp]
        L.twin_selfplay.restype = i64
        L.twin_selfplay.argtypes = [i64, u64, u64, u64, i32, u64, u64, u64, i32, u64, i32, i32, i64, i64, vp, vp, vp, i64, vp, vp,
                                    vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def e6(x):
    """The option value of a real eps / alpha (what Engine.set_root_noise sends)."""
    return int(round(float(x) * 1e6))


def default_reserve(sims):
    return 8 + 42 * (7 * sims + 8)


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


class Tree:
    """One AsyncMcts of the oracle whose get_action_prob mixes root noise in first."""

    def __init__(self, sims, net_kind=NET_STUB, salt=0, cpuct=1, max_depth=1000, reserve=None, model_id=0, game_kind=GAME_BITS, threads=1):
        self._keep = None
        self._h = lib().twin_tree_new(game_kind, reserve or default_reserve(sims), sims, threads, max_depth, model_id, cpuct, net_kind, salt)
        if not self._h:
            raise RuntimeError("twin_tree_new failed")

    def get_action_prob(self, mine, theirs, temp, seed=0, game_id=0, eps=0.0, alpha=1.0):
        pi, counts, q = np.zeros(7, np.float32), np.zeros(7, np.uint16), np.zeros(7, np.float32)
        rc = lib().twin_tree_get_action_prob(self._h, int(mine), int(theirs), temp, seed, game_id, e6(eps), e6(alpha), _p(pi), _p(counts), _p(q))
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
             game_kind=GAME_BITS, replay=None, sim_threads=1, eps=0.0, alpha=1.0):
    """Coach::execute_episode x n_games with root noise; the result has the fields of oracle_py.selfplay."""
    cap = n_games * 84
    boards, pis, zs = np.zeros((cap, 2, 6, 7), np.float32), np.zeros((cap, 7), np.float32), np.zeros(cap, np.float32)
    game_len, moves, bad = np.zeros(n_games, np.int32), np.zeros((n_games, 42), np.uint8), np.zeros(n_games, np.int32)
    ro = rs = rp = rv = None
    if replay is not None:
        ro = np.ascontiguousarray(replay[0], np.int64)
        rs = None if replay[1] is None else np.ascontiguousarray(replay[1], np.uint64)
        rp, rv = np.ascontiguousarray(replay[2], np.float32), np.ascontiguousarray(replay[3], np.float32)
    n = lib().twin_selfplay(n_games, first_game_id, sims, temp_threshold, cpuct, max_depth, reserve or default_reserve(sims), seed, net_kind, salt,
                            game_kind, sim_threads, e6(eps), e6(alpha), _p(boards), _p(pis), _p(zs), cap, _p(game_len), _p(moves),
                            _p(ro), _p(rs), _p(rp), _p(rv), _p(bad))
    if n < 0:
        raise RuntimeError("twin selfplay failed")
    return {"count": int(n), "game_len": game_len, "moves": moves, "replay_bad": bad, "boards": boards[:n], "pis": pis[:n], "zs": zs[:n]}
