"""Search statistics as training targets without a GPU (csrc/az_target.h): the g++ build of the rule header against
numpy f32 / f64 restatements -- root value, z/q blend, KL, copies --, the root value's sign on two positions searched by the self-play
twin, and the host-only paths of the two Coaches."""
import math
import os
import subprocess

import numpy as np
import pytest

import selfplay_twin as tw
import target_twin as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH_SALT = 1234
COPY_SIZES = (1, 2, 257, 2047, 2048, 2049, 5000)      # one tuple, the workgroup edge, the 2048-wide scan block edge of az_draw.h


def bits(*cells):
    return sum(1 << c for c in cells)


# ---- 1. the root value --------------------------------------------------------------------------------------------------------------------
ROOT_CASES = [
    ([10, 0, 5, 0, 0, 0, 1], [0.25, 0.0, -0.5, 0.0, 0.0, 0.0, 1.01]),
    ([0, 0, 0, 50, 0, 0, 0], [0.0, 0.0, 0.0, 1.01, 0.0, 0.0, 0.0]),           # a single child that wins at once: q = 1.01 is clamped
    ([0, 0, 0, 0, 0, 0, 0], [0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3]),             # N = 0
    ([0, 7, 0, 0, 0, 0, 0], [0.9, -0.123456, 0.9, 0.9, 0.9, 0.9, 0.9]),       # a single child; the q of unvisited ones is not read
    ([3, 3, 3, 3, 3, 3, 3], [-1.01, -1.01, -1.01, -1.01, -1.01, -1.01, -1.01]),
    ([65535, 65535, 1, 2, 3, 4, 5], [0.1, -0.1, 0.7, 0.3, -0.9, 0.5, 0.001]),
]


def test_root_value_against_numpy_f32():
    counts = np.array([c for c, _ in ROOT_CASES], np.uint32)
    q = np.array([x for _, x in ROOT_CASES], np.float32)
    got = tt.root_value(counts, q)
    want = np.array([tt.root_value_py(c, x) for c, x in zip(counts, q)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[1] == 1.0 and got[2] == 0.0 and got[4] == -1.0
    assert got[3] == np.float32(np.float32(np.float32(7) * np.float32(-0.123456)) / np.float32(7))
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 200, (500, 7)).astype(np.uint32) * (rng.random((500, 7)) < 0.7)
    q = rng.uniform(-1.01, 1.01, (500, 7)).astype(np.float32)
    got = tt.root_value(counts, q)
    want = np.array([tt.root_value_py(c, x) for c, x in zip(counts, q)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(np.abs(got) <= 1.0)


@pytest.mark.parametrize("mine,theirs,sims,sign", [(bits(0, 7, 14), bits(1, 8, 15), 50, +1), (bits(15, 22, 23), bits(14, 21, 28), 200, -1)])
def test_root_value_has_the_sign_of_the_side_to_move(mine, theirs, sims, sign):
    """The mover wins with column 3 / every move loses to an open three (hash net, salt 1234, seed 3, game id 7): R > 0.5 / R < -0.5
    from the twin's raw counts and q."""
    t = tw.Tree(sims, net_kind=tw.NET_HASH, salt=HASH_SALT)
    _, counts, q = t.get_action_prob(mine, theirs, 1.0, seed=3, game_id=7)
    t.close()
    R = float(tt.root_value(counts, q)[0])
    print("R = %.3f at %d simulations" % (R, sims))
    assert R == float(tt.root_value_py(counts, q))
    assert sign * R > 0.5 and abs(R) <= 1.0


# ---- 2. the blend -------------------------------------------------------------------------------------------------------------------------
def test_blend_against_numpy_f32():
    rng = np.random.default_rng(5)
    z = rng.choice(np.array([-1.0, 1.0, -1e-4, 1e-4, 0.0, -0.0], np.float32), 400)
    r = rng.uniform(-1, 1, 400).astype(np.float32)
    for lam in (0.0, 1.0, 0.5, 0.25, 0.333333, 0.999999, 0.000001):
        got = tt.blend(z, r, lam)
        want = np.array([tt.blend_py(a, b, lam) for a, b in zip(z, r)], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), lam
        assert np.all(np.abs(got) <= 1.0)
    assert np.array_equal(tt.blend(z, r, 0.0).view(np.uint32), z.view(np.uint32))          # bit for bit, signed zeros included
    assert np.array_equal(tt.blend(z, r, 1.0).view(np.uint32), r.view(np.uint32))


# ---- 3. the surprise ----------------------------------------------------------------------------------------------------------------------
def kl_inputs():
    pis, priors = tt.copy_inputs(3000)
    hand_pi = np.array([[1, 0, 0, 0, 0, 0, 0], [0.5, 0.5, 0, 0, 0, 0, 0], [1 / 7] * 7, [0, 0, 0, 1, 0, 0, 0], [1e-30, 1 - 1e-30, 0, 0, 0, 0, 0],
                        [0, 0, 0, 0, 0, 0, 0], [0.25, 0.25, 0.25, 0.25, 0, 0, 0]], np.float32)
    hand_pr = np.array([[1, 0, 0, 0, 0, 0, 0], [0.5, 0.5, 0, 0, 0, 0, 0], [1 / 7] * 7, [0, 0, 0, 0, 1, 0, 0], [0.5, 0.5, 0, 0, 0, 0, 0],
                        [1 / 7] * 7, [1e-40, 0.5, 0.25, 0.25, 0, 0, 0]], np.float32)
    return np.concatenate([pis, hand_pi]), np.concatenate([priors, hand_pr])


def test_kl_against_float64():
    """|KL - KL_f64| <= 1e-6 * (1 + sum_a pi_a (|log2 pi_a| + |log2 max(prior_a, 2^-126)|)): noise_log2's documented 2.7e-7 relative error
    on each of two logs, plus the f32 roundings of three operations per term and seven additions."""
    pis, priors = kl_inputs()
    got, K, SK = tt.kl(pis, priors)
    worst = 0.0
    for i in range(len(pis)):
        want, scale = tt.kl_f64(pis[i], priors[i])
        bound = 1e-6 * (1.0 + scale)
        worst = max(worst, abs(float(got[i]) - want) / bound)
        assert abs(float(got[i]) - want) <= bound, (i, got[i], want, bound)
    print("largest |error| / bound = %.3f" % worst)
    assert np.all(got >= 0.0) and np.all(got <= 64.0)
    assert got[-7] == 0.0 and got[-6] == 0.0 and got[-5] == 0.0 and got[-2] == 0.0      # pi == prior, and an all-zero pi
    assert got[-4] == 64.0                                                               # a prior of 0 under pi = 1: 126 ln 2 is clamped
    assert np.array_equal(K, np.array([int(np.rint(float(x) * 2.0 ** 32)) for x in got], np.uint64))
    assert SK == int(K.astype(object).sum())


@pytest.mark.parametrize("share", [0.5, 1.0])
@pytest.mark.parametrize("n", COPY_SIZES)
def test_copies(n, share):
    """The g++ build against the Python-float restatement; the total stays within 2.5 sqrt(n) + 1 of n (a float64 simulation of the rule
    gives differences of 0 to 26 against bounds of 3.5 to 178); sum c_i <= 2n; the expanded set is np.repeat of the input."""
    pis, priors = tt.copy_inputs(n)
    r = tt.surprise(pis, priors, share, 1)
    _, K, SK = tt.kl(pis, priors)
    assert np.array_equal(r["counts"], tt.copies_py(K, share, 1))
    total = int(r["counts"].sum())
    print("n %d share %.1f: sum c_i = %d (bound %.1f), largest c_i %d" % (n, share, total, 2.5 * math.sqrt(n) + 1, int(r["counts"].max())))
    assert total == r["total"]
    assert abs(total - n) <= 2.5 * math.sqrt(n) + 1
    assert total <= 2 * n
    if SK:
        assert abs(float(r["w"].sum()) - n) <= 1e-9 * n
    zs = np.arange(n, dtype=np.float32)
    ep, ez = tt.expand(r["counts"], pis, zs)
    assert len(ez) == total and np.array_equal(ez, np.repeat(zs, r["counts"])) and np.array_equal(ep, np.repeat(pis, r["counts"], axis=0))
    assert np.all(np.diff(ez) >= 0)                              # input order
    assert np.array_equal(np.bincount(ez.astype(np.int64), minlength=n), r["counts"])


@pytest.mark.parametrize("n", COPY_SIZES)
def test_copies_are_all_one_without_surprise(n):
    pis, priors = tt.copy_inputs(n)
    assert np.array_equal(tt.surprise(pis, pis, 1.0, 1)["counts"], np.ones(n, np.uint32))            # pi == prior everywhere: SK = 0
    assert tt.kl(pis, pis)[2] == 0
    assert np.array_equal(tt.surprise(pis, priors, 0.0, 1)["counts"], np.ones(n, np.uint32))         # share = 0


def test_surprising_tuples_get_more_copies():
    pis, priors = tt.copy_inputs(5000)
    r = tt.surprise(pis, priors, 1.0, 1)
    order = np.argsort(r["kl"])
    assert r["counts"][order[-500:]].sum() > 4 * r["counts"][order[:500]].sum()
    assert np.all(r["counts"][r["kl"] == 0] == 0)               # share 1: a tuple that did not surprise is not written


# ---- 4. the hosts ---------------------------------------------------------------------------------------------------------------------------
def test_python_coach_targets_host_paths():
    """The record option holds around self-play only; surprise_share with a world of 2 raises before the engine is asked."""
    import alphazero_rs_amd.coach as coach_mod
    calls = []

    class FakeEngine:
        def set_option(self, key, value):
            calls.append((key, value))

    c = coach_mod.Coach.__new__(coach_mod.Coach)
    c.engine = FakeEngine()
    c.value_target_q, c.surprise_share = 0.5, 0.0
    with c._selfplay_record_search():
        calls.append(("selfplay",))
    assert calls == [("selfplay_record_search", 1), ("selfplay",), ("selfplay_record_search", 0)]
    c.value_target_q, c.surprise_share = 0.0, 0.0
    calls.clear()
    with c._selfplay_record_search():
        calls.append(("selfplay",))
    assert calls == [("selfplay",)]
    c.surprise_share, c.num_eps = 0.5, 8
    c._world = lambda: (0, 2)
    calls.clear()
    with pytest.raises(ValueError, match="world of 1"):
        c.execute_episodes(0, 0, 1)
    assert calls == []
    c.surprise_share, c.value_target_q = 0.0, 1.5
    with pytest.raises(ValueError, match="0 .. 1"):
        c.execute_episodes(0, 0, 1)


def test_cpp_coach_targets_host_paths(tmp_path):
    exe = str(tmp_path / "test_targets_host_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_targets_host_cpu.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe, str(tmp_path / "coach")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
