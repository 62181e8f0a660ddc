"""The rule of csrc/az_target.h -- root value, z/q blend, KL surprise and copies -- as its g++ build
(tests/cpp/target_twin.cpp) behind ctypes, plus restatements with numpy f32 / f64 that the CPU tests hold the build to.
TEST INFRASTRUCTURE ONLY.  The library is compiled once per process into a temporary directory (g++ -O2 -ffp-contract=off, the flags the
header states)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
RNG_SURPRISE = 10
MIN_NORMAL = np.float32(2.0 ** -126)

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="target_twin_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libtarget_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "target_twin.cpp"), "-o", so])
        L = C.CDLL(so)
        u64, i64, vp = C.c_uint64, C.c_int64, C.c_void_p
        L.twin_root_value.restype = None; L.twin_root_value.argtypes = [i64, vp, vp, vp]
        L.twin_blend.restype = None; L.twin_blend.argtypes = [i64, vp, vp, i64, vp]
        L.twin_kl.restype = u64; L.twin_kl.argtypes = [i64, vp, vp, vp, vp]
        L.twin_surprise.restype = u64; L.twin_surprise.argtypes = [i64, vp, vp, i64, u64, vp, vp, vp]
        L.twin_rng_surprise.restype = u64; L.twin_rng_surprise.argtypes = []
        assert L.twin_rng_surprise() == RNG_SURPRISE
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def e6(x):
    return int(round(float(x) * 1e6))


# ---- the g++ build --------------------------------------------------------------------------------------------------------------------------
def root_value(counts, q):
    """R [n] f32 of counts [n,7] and q [n,7] (a single row may be given as [7])."""
    c = np.ascontiguousarray(counts, np.uint32).reshape(-1, 7)
    qq = np.ascontiguousarray(q, np.float32).reshape(-1, 7)
    assert len(c) == len(qq)
    out = np.zeros(len(c), np.float32)
    lib().twin_root_value(len(c), _p(c), _p(qq), _p(out))
    return out


def blend(zs, root_q, lam):
    z = np.ascontiguousarray(zs, np.float32).reshape(-1)
    r = np.ascontiguousarray(root_q, np.float32).reshape(-1)
    assert len(z) == len(r)
    out = np.zeros(len(z), np.float32)
    lib().twin_blend(len(z), _p(z), _p(r), e6(lam), _p(out))
    return out


def kl(pis, priors):
    """(kl [n] f32, K [n] u64, SK)."""
    p = np.ascontiguousarray(pis, np.float32).reshape(-1, 7)
    r = np.ascontiguousarray(priors, np.float32).reshape(-1, 7)
    assert len(p) == len(r)
    out, K = np.zeros(len(p), np.float32), np.zeros(len(p), np.uint64)
    sk = lib().twin_kl(len(p), _p(p), _p(r), _p(out), _p(K))
    return out, K, int(sk)


def surprise(pis, priors, share, seed):
    """dict(counts [n] u32, kl [n] f32, w [n] f64, total)."""
    p = np.ascontiguousarray(pis, np.float32).reshape(-1, 7)
    r = np.ascontiguousarray(priors, np.float32).reshape(-1, 7)
    assert len(p) == len(r)
    n = len(p)
    counts, out, w = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.float64)
    total = lib().twin_surprise(n, _p(p), _p(r), e6(share), int(seed) & M64, _p(counts), _p(out), _p(w))
    return {"counts": counts, "kl": out, "w": w, "total": int(total)}


def expand(counts, *arrays):
    """The expanded set: every array's rows repeated by counts, in input order."""
    c = np.asarray(counts, np.int64)
    return tuple(np.repeat(np.asarray(a), c, axis=0) for a in arrays)


# ---- restatements -------------------------------------------------------------------------------------------------------------------------------
def root_value_py(counts, q):
    """The rule with numpy f32, every operation rounding once."""
    f = np.float32
    acc, N = f(0.0), 0
    for n, x in zip(np.asarray(counts, np.int64), np.asarray(q, np.float32)):
        if n > 0:
            acc = f(acc + f(f(n) * f(x)))
            N += int(n)
    if N == 0:
        return f(0.0)
    return f(min(max(f(acc / f(N)), f(-1.0)), f(1.0)))


def blend_py(z, r, lam):
    f = np.float32
    l6 = e6(lam)
    if l6 == 0:
        return f(z)
    if l6 == 1000000:
        return f(r)
    b = f(f(l6) / f(1e6))
    a = f(f(1.0) - b)
    return f(f(a * f(z)) + f(b * f(r)))


def kl_f64(pi, prior):
    """(KL in float64 from the f32 inputs, the scale sum_a pi_a (|log2 pi_a| + |log2 max(prior_a, 2^-126)|) of its error bound)."""
    p = np.asarray(pi, np.float32).astype(np.float64)
    r = np.maximum(np.asarray(prior, np.float32), MIN_NORMAL).astype(np.float64)
    m = np.asarray(pi, np.float32) >= MIN_NORMAL
    kl = float(np.sum(p[m] * (np.log(p[m]) - np.log(r[m]))))
    scale = float(np.sum(p[m] * (np.abs(np.log2(p[m])) + np.abs(np.log2(r[m])))))
    return min(max(kl, 0.0), 64.0), scale


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rng_draw(seed, i, j, purpose):
    return mix64(mix64(mix64(mix64(seed) ^ i) ^ j) ^ purpose)


def copies_py(K, share, seed):
    """counts [n] from the fixed-point K [n] with Python floats (IEEE double, one rounding per operation)."""
    K = [int(k) for k in K]
    n, SK, s = len(K), sum(K), e6(share) / 1e6
    out = np.zeros(n, np.uint32)
    for i, k in enumerate(K):
        w = 1.0 if SK == 0 else (1.0 - s) + s * ((float(n) * float(k)) / float(SK))
        u = float(rng_draw(seed, i, 0, RNG_SURPRISE) >> 11) * 2.0 ** -53
        fl = float(np.floor(w))
        out[i] = int(fl) + (1 if u < w - fl else 0)
    return out


def copy_inputs(n):
    """The inputs the issue fixes for the copies tests: pis ~ Dirichlet(0.5), priors ~ Dirichlet(1), in that order from default_rng(7)."""
    rng = np.random.default_rng(7)
    pis = rng.dirichlet(0.5 * np.ones(7), n).astype(np.float32)
    priors = rng.dirichlet(np.ones(7), n).astype(np.float32)
    return pis, priors
