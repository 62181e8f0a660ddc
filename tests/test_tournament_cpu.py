"""az_rating_fit (alphazero-rs_amd/csrc/az_rating.h through the C ABI) without a GPU: against the pure-Python twin of the same steps
(tests/rating_twin.py), the closed form at K = 2, the fixed-point equation, relabelling and the refusals; and the header compiled alone by
g++ with AddressSanitizer and UBSan, run as a stand-alone program (tests/cpp/rating_fit.cpp)."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import rating_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9      # the arithmetic is the twin's, operation for operation: only log10 and sqrt may differ


def random_matrix(K, seed, lo=0, hi=40, missing=()):
    rng = np.random.default_rng(seed)
    wld = np.zeros((K, K, 3), np.uint64)
    for i in range(K):
        for j in range(i + 1, K):
            if (i, j) in missing:
                continue
            w, l, d = (int(x) for x in rng.integers(lo, hi, 3))
            wld[i, j] = (w, l, d)
            wld[j, i] = (l, w, d)
    return wld


def sweep_matrix(K, winner, games=20):
    """Model `winner` wins every game it plays; the others draw among themselves."""
    wld = np.zeros((K, K, 3), np.uint64)
    for i in range(K):
        for j in range(K):
            if i != j:
                wld[i, j] = (games, 0, 0) if i == winner else ((0, games, 0) if j == winner else (0, 0, games))
    return wld


CASES = {
    "random_k2": (random_matrix(2, 1), 2.0),
    "random_k3": (random_matrix(3, 2), 2.0),
    "random_k8": (random_matrix(8, 3), 2.0),
    "random_k16": (random_matrix(16, 4), 2.0),
    "random_k8_no_prior": (random_matrix(8, 5, lo=1), 0.0),
    "all_draws": (sweep_matrix(5, winner=-1), 2.0),
    "sweep_by_one": (sweep_matrix(6, winner=2), 2.0),
    "missing_pairs": (random_matrix(6, 6, missing={(0, 3), (1, 2), (4, 5)}), 2.0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_matches_the_twin(engine_mod, name):
    wld, prior = CASES[name]
    elo, se, sweeps = engine_mod.rating_fit(wld, prior)
    t_elo, t_se, t_sweeps, _ = rating_twin.rating_fit(wld.tolist(), prior)
    print(name, "sweeps", sweeps, "elo", elo.tolist(), "se", se.tolist())
    assert sweeps == t_sweeps and 1 <= sweeps < rating_twin.MAX_SWEEPS
    assert np.max(np.abs(elo - np.array(t_elo))) <= TOL
    assert np.max(np.abs(se - np.array(t_se))) <= TOL
    assert abs(float(np.sum(elo))) <= TOL and np.all(se > 0)
    if name == "all_draws":
        assert np.max(np.abs(elo)) <= 1e-12
    if name == "sweep_by_one":
        assert int(np.argmax(elo)) == 2 and np.max(np.abs(np.delete(elo, 2) - np.delete(elo, 2)[0])) <= TOL


@pytest.mark.parametrize("w,l,d,prior", [(7, 3, 2, 2.0), (30, 1, 0, 2.0), (0, 9, 5, 2.0), (11, 11, 4, 0.0), (5, 2, 1, 0.5)])
def test_closed_form_at_k2(engine_mod, w, l, d, prior):
    wld = np.zeros((2, 2, 3), np.uint64)
    wld[0, 1], wld[1, 0] = (w, l, d), (l, w, d)
    elo, _, _ = engine_mod.rating_fit(wld, prior)
    s = (w + d / 2.0 + prior / 2.0) / (w + l + d + prior)
    assert abs((elo[0] - elo[1]) - 400.0 * math.log10(s / (1.0 - s))) <= TOL


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixed_point(engine_mod, name):
    """sum_j n_ij gamma_i / (gamma_i + gamma_j) = S_i for every model, gamma recovered from elo up to the common factor (which cancels)."""
    wld, prior = CASES[name]
    elo, _, _ = engine_mod.rating_fit(wld, prior)
    K = len(elo)
    g = [10.0 ** (x / 400.0) for x in elo]
    for i in range(K):
        S = lhs = 0.0
        for j in range(K):
            if j != i:
                W, L, D = (float(x) for x in wld[i, j])
                S += W + D / 2.0 + prior / 2.0
                lhs += (W + L + D + prior) * g[i] / (g[i] + g[j])
        assert abs(lhs - S) <= 1e-9 * S, (i, lhs, S)


@pytest.mark.parametrize("name", ["random_k8", "missing_pairs", "sweep_by_one"])
def test_relabelling_permutes_the_ratings(engine_mod, name):
    wld, prior = CASES[name]
    K = wld.shape[0]
    perm = np.random.default_rng(9).permutation(K)
    elo, se, _ = engine_mod.rating_fit(wld, prior)
    elo_p, se_p, _ = engine_mod.rating_fit(wld[np.ix_(perm, perm)], prior)
    assert np.max(np.abs(elo_p - elo[perm])) <= TOL and np.max(np.abs(se_p - se[perm])) <= TOL


def test_refusals_write_nothing(engine_mod):
    lib = C.CDLL(engine_mod.LIB_PATH)
    lib.az_rating_fit.restype = C.c_int32
    lib.az_rating_fit.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    wld = random_matrix(16, 7)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good = (wld, 4, 2.0)
    for K, prior, null in ((1, 2.0, None), (17, 2.0, None), (0, 2.0, None), (-3, 2.0, None), (4, -0.5, None), (4, float("inf"), None),
                           (4, float("nan"), None), (4, 2.0, "wld"), (4, 2.0, "elo")):
        elo, se, sweeps = np.full(17, 77.0), np.full(17, 77.0), np.full(1, 77, np.int32)
        st = lib.az_rating_fit(None if null == "wld" else ptr(wld), K, prior, None if null == "elo" else ptr(elo), ptr(se), ptr(sweeps))
        assert st == 1, (K, prior, null)
        assert np.all(elo == 77.0) and np.all(se == 77.0) and sweeps[0] == 77
    elo, sweeps = np.full(17, 77.0), np.full(1, 77, np.int32)
    assert lib.az_rating_fit(ptr(good[0][:4, :4].copy()), good[1], good[2], ptr(elo), None, None) == 0      # elo_se and sweeps may be NULL
    assert np.all(elo[4:] == 77.0) and not np.any(elo[:4] == 77.0)
    with pytest.raises(engine_mod.AzError):
        engine_mod.rating_fit(wld[:4, :4], -1.0)


def test_header_alone_under_sanitizers(tmp_path):
    """csrc/az_rating.h is host-only: g++ compiles it alone, and the stand-alone program runs clean under ASan + UBSan and agrees with
    the twin."""
    exe = os.path.join(tmp_path, "rating_fit")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "rating_fit.cpp"), "-o", exe])
    assert subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip() == "ok"
    for name in ("random_k3", "random_k16", "missing_pairs"):
        wld, prior = CASES[name]
        args = [exe, str(wld.shape[0]), repr(prior)] + [str(int(x)) for x in wld.reshape(-1)]
        got = json.loads(subprocess.run(args, check=True, stdout=subprocess.PIPE, text=True).stdout)
        t_elo, t_se, t_sweeps, _ = rating_twin.rating_fit(wld.tolist(), prior)
        assert got["sweeps"] == t_sweeps
        assert max(abs(a - b) for a, b in zip(got["elo"], t_elo)) <= TOL and max(abs(a - b) for a, b in zip(got["elo_se"], t_se)) <= TOL
