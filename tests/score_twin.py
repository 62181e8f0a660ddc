"""The rule of csrc/az_score.h -- the per-tuple score with its integer sums, the hold-out rule and the best / stop decision (DESIGN.md
sections 4.1l and 8.3) -- as its g++ build (tests/cpp/score_twin.cpp) behind ctypes, plus an independent restatement with numpy f32 /
Python integers that the CPU tests hold the build to and the GPU tests hold the kernels to.  TEST INFRASTRUCTURE ONLY.  The library is
compiled once per process into a temporary directory (g++ -O2 -ffp-contract=off, the flags the header states)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
MIN_NORMAL = np.float32(2.0 ** -126)
LN2 = np.float32(0.693147182)
ONE = 1073741824.0            # 2^30

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="score_twin_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libscore_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "score_twin.cpp"), "-o", so])
        L = C.CDLL(so)
        u64, i64, i32, vp = C.c_uint64, C.c_int64, C.c_int32, C.c_void_p
        L.twin_score.restype = None; L.twin_score.argtypes = [i64] + [vp] * 11
        L.twin_holdout.restype = None; L.twin_holdout.argtypes = [i64, vp, i64, u64, vp, vp]
        L.twin_best_stop.restype = i32; L.twin_best_stop.argtypes = [vp, i32, i32, C.POINTER(i32)]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def e6(x):
    return int(round(float(x) * 1e6))


def results(sums):
    """(loss_pi, loss_v, kl, top1) as doubles from the integers (S_ce, S_kl, S_se, S_hit, W)."""
    s_ce, s_kl, s_se, s_hit, w = (int(x) for x in sums)
    return (float(s_ce) / ONE / float(w), float(s_se) / ONE / float(w), float(s_kl) / ONE / float(w), float(s_hit) / float(w))


def _inputs(p, v, pis, zs, states, weights):
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 7)
    n = len(p)
    v = np.ascontiguousarray(v, np.float32).reshape(n)
    pis = np.ascontiguousarray(pis, np.float32).reshape(n, 7)
    zs = np.ascontiguousarray(zs, np.float32).reshape(n)
    states = np.ascontiguousarray(states, np.uint64).reshape(n, 2)
    weights = None if weights is None else np.ascontiguousarray(weights, np.uint32).reshape(n)
    return n, p, v, pis, zs, states, weights


# ---- the g++ build --------------------------------------------------------------------------------------------------------------------------
def score(p, v, pis, zs, states, weights=None):
    """dict(sums (5 ints), ce, se, kl [n] f32, hit [n] u8) of the net output (p [n,7], v [n]) against (pis, zs) on states [n,2]."""
    n, p, v, pis, zs, states, weights = _inputs(p, v, pis, zs, states, weights)
    sums = np.zeros(5, np.uint64)
    ce, se, kl = (np.zeros(n, np.float32) for _ in range(3))
    hit = np.zeros(n, np.uint8)
    lib().twin_score(n, _p(p), _p(v), _p(pis), _p(zs), _p(states), _p(weights), _p(sums), _p(ce), _p(se), _p(kl), _p(hit))
    return {"sums": tuple(int(x) for x in sums), "ce": ce, "se": se, "kl": kl, "hit": hit}


def holdout(states, share, seed):
    """(held [n] bool, keys [n] u64)."""
    s = np.ascontiguousarray(states, np.uint64).reshape(-1, 2)
    held, keys = np.zeros(len(s), np.uint8), np.zeros(len(s), np.uint64)
    lib().twin_holdout(len(s), _p(s), e6(share), int(seed) & M64, _p(held), _p(keys))
    return held.astype(bool), keys


def best_stop(hist, patience):
    """(best epoch, stop) behind the last row of hist [n,4]."""
    h = np.ascontiguousarray(hist, np.float64).reshape(-1, 4)
    best = C.c_int32(-1)
    stop = lib().twin_best_stop(_p(h), len(h), int(patience), C.byref(best))
    return int(best.value), bool(stop)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def log2_np(x):
    """noise_log2 of csrc/az_noise.h on an f32 array, every operation rounding once to f32."""
    f = np.float32
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    e = (u >> 23) - 127
    mb = (u & 0x007FFFFF) | 0x3F800000
    big = mb >= 0x3FB504F3
    mb = np.where(big, mb - 0x00800000, mb)
    e = np.where(big, e + 1, e)
    m = mb.astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        s = (m - f(1.0)) / (m + f(1.0))
        z = s * s
        p = np.full_like(s, f(0.111111111))
        for c in (0.142857143, 0.2, 0.333333333, 1.0):
            p = p * z + f(c)
        ln_m = (f(2.0) * s) * p
        return e.astype(np.float32) + ln_m * f(1.44269504)


def _masked_sum(terms, mask):
    """t = 0; for a ascending where mask: t = t + terms[a], in f32."""
    t = np.zeros(len(terms), np.float32)
    with np.errstate(all="ignore"):
        for a in range(7):
            t = np.where(mask[:, a], t + terms[:, a], t)
    return t


def ce_np(pis, p):
    f = np.float32
    with np.errstate(all="ignore"):
        q = np.where(p > MIN_NORMAL, p, MIN_NORMAL).astype(np.float32)
        t = _masked_sum(pis * log2_np(q), pis >= MIN_NORMAL)
        ce = -(t * LN2)
        return np.where(np.isnan(ce), f(128.0), np.where(ce > f(0.0), np.minimum(ce, f(128.0)), f(0.0))).astype(np.float32)


def kl_np(pis, p):
    """target_kl of csrc/az_target.h."""
    f = np.float32
    with np.errstate(all="ignore"):
        q = np.where(p > MIN_NORMAL, p, MIN_NORMAL).astype(np.float32)
        safe = np.where(pis >= MIN_NORMAL, pis, f(1.0)).astype(np.float32)
        t = _masked_sum(pis * (log2_np(safe) - log2_np(q)), pis >= MIN_NORMAL)
        kl = t * LN2
        return np.where(kl >= f(0.0), np.minimum(kl, f(64.0)), f(0.0)).astype(np.float32)


def se_np(v, zs):
    with np.errstate(all="ignore"):
        d = v - zs
        se = d * d
        return np.where(se <= np.float32(4.0), se, np.float32(4.0)).astype(np.float32)


def hit_np(pis, p, states):
    out = np.zeros(len(p), np.uint8)
    for i in range(len(p)):
        occ = int(states[i, 0]) | int(states[i, 1])
        ts = int(np.argmax(pis[i]))                                    # the first maximum
        ms, best = -1, None
        for a in range(7):
            if (occ >> (a * 7 + 5)) & 1 or np.isnan(p[i, a]):
                continue
            if ms < 0 or p[i, a] > best:
                ms, best = a, p[i, a]
        out[i] = 1 if ts == ms else 0
    return out


def fixed(x):
    """K(x) = llrint((double)x * 2^30) as Python integers (np.rint rounds halves to even, as llrint does)."""
    return [int(k) for k in np.rint(np.asarray(x, np.float32).astype(np.float64) * ONE)]


def score_py(p, v, pis, zs, states, weights=None):
    n, p, v, pis, zs, states, weights = _inputs(p, v, pis, zs, states, weights)
    w = [1] * n if weights is None else [int(x) for x in weights]
    ce, kl, se, hit = ce_np(pis, p), kl_np(pis, p), se_np(v, zs), hit_np(pis, p, states)
    sums = (sum(wi * k for wi, k in zip(w, fixed(ce))), sum(wi * k for wi, k in zip(w, fixed(kl))), sum(wi * k for wi, k in zip(w, fixed(se))),
            sum(wi * int(h) for wi, h in zip(w, hit)), sum(w))
    return {"sums": sums, "ce": ce, "se": se, "kl": kl, "hit": hit}


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def mirror_bits(b):
    return sum(((b >> (c * 7)) & 0x7F) << ((6 - c) * 7) for c in range(7))


BOTTOM = sum(1 << (7 * c) for c in range(7))


def holdout_key_py(mine, theirs):
    """The pack word of the mirror-canonical state: the smaller of the position's and its mirror image's."""
    k = mine + (mine | theirs) + BOTTOM
    mm, mt = mirror_bits(mine), mirror_bits(theirs)
    return min(k, mm + (mm | mt) + BOTTOM)


def holdout_py(states, share, seed):
    thresh = (e6(share) << 24) // 1000000
    s = np.asarray(states, np.uint64).reshape(-1, 2)
    return np.array([(mix64(mix64(int(seed) & M64) ^ holdout_key_py(int(a), int(b))) >> 40) < thresh for a, b in s], bool)


def best_stop_py(hist, patience):
    sums = [float(r[0]) + float(r[1]) for r in hist]
    best = 0
    for k, s in enumerate(sums):
        if s == s and (sums[best] != sums[best] or s < sums[best]):
            best = k
    return best, patience > 0 and len(sums) - 1 - best >= patience


# ---- positions ------------------------------------------------------------------------------------------------------------------------------
def random_states(n, seed, distinct=False):
    """n positions of random legal play (no winner check: a state is whatever stones stack to), as [n,2] u64 (mine, theirs)."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        mine = theirs = 0
        for _ in range(int(rng.integers(0, 30))):
            occ = mine | theirs
            cols = [c for c in range(7) if not (occ >> (c * 7 + 5)) & 1]
            if not cols:
                break
            c = int(rng.choice(cols))
            bit = (occ + (1 << (c * 7))) & (0x3F << (c * 7))
            mine, theirs = theirs, mine | bit
        key = holdout_key_py(mine, theirs)
        if distinct and key in seen:
            continue
        seen.add(key)
        out.append((mine, theirs))
    return np.array(out, np.uint64)


def mirror_states(states):
    s = np.asarray(states, np.uint64).reshape(-1, 2)
    return np.array([(mirror_bits(int(a)), mirror_bits(int(b))) for a, b in s], np.uint64)
