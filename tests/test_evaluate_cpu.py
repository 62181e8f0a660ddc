"""CPU tests of the held-out score (csrc/az_score.h; DESIGN.md sections 4.1l and 8.3): the g++ build of the header against an independent
numpy restatement on random and edge tuples, the hold-out rule, the best / stop decision, the new exports, and the Python Coach's split on a
fake engine.  Every comparison is bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import score_twin as tw

TINY = np.float32(2.0 ** -126)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_score(got, want):
    assert got["sums"] == tuple(want["sums"])
    for k in ("ce", "se", "kl"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(got["hit"], want["hit"])


def random_tuples(n, seed):
    g = np.random.default_rng(seed)
    p = g.dirichlet(0.3 * np.ones(7), n).astype(np.float32)
    pis = g.dirichlet(0.3 * np.ones(7), n).astype(np.float32)
    pis[g.random((n, 7)) < 0.2] = 0.0                                  # pruned actions
    onehot = g.random(n) < 0.2
    pis[onehot] = np.eye(7, dtype=np.float32)[g.integers(0, 7, int(onehot.sum()))]
    v = g.uniform(-1, 1, n).astype(np.float32)
    zs = np.where(g.random(n) < 0.5, g.choice([-1.0, 0.0, 1.0], n), g.uniform(-1, 1, n)).astype(np.float32)
    return p, v, pis, zs, tw.random_states(n, seed + 1)


def test_build_equals_restatement_on_random_tuples():
    p, v, pis, zs, states = random_tuples(3000, 5)
    w = np.random.default_rng(6).integers(0, 6, len(v)).astype(np.uint32)
    for weights in (None, w):
        got, want = tw.score(p, v, pis, zs, states, weights), tw.score_py(p, v, pis, zs, states, weights)
        assert_same_score(got, want)
    assert 0 < got["sums"][3] < got["sums"][4] == int(w.sum())
    assert tw.results(got["sums"])[0] > 0


def full_columns(cols):
    """A state whose columns `cols` are full (stones alternate from the bottom)."""
    mine = theirs = 0
    for c in cols:
        for r in range(6):
            if r % 2 == 0:
                mine |= 1 << (c * 7 + r)
            else:
                theirs |= 1 << (c * 7 + r)
    return mine, theirs


def test_edge_tuples():
    nan = np.float32(np.nan)
    u = np.full(7, 1 / 7, np.float32)
    rows = []      # (p, v, pi, z, state, weight)
    rows.append((u, 0.5, np.eye(7, dtype=np.float32)[3], 1.0, (0, 0), 1))                                  # one-hot pi
    rows.append((u, -0.25, np.zeros(7, np.float32), -1.0, (0, 0), 1))                                      # all-zero pi: ce = kl = 0
    rows.append((np.array([0, 1e-45, 1e-39, TINY, 0.5, 0.25, 0.25], np.float32), 0.0, u, 0.0, (0, 0), 1))  # p below 2^-126: floored
    rows.append((np.array([nan, 0.2, 0.2, 0.2, 0.2, 0.1, 0.1], np.float32), 0.0, u, 0.5, (0, 0), 1))       # NaN p: floored, never m*
    rows.append((np.full(7, nan, np.float32), nan, np.eye(7, dtype=np.float32)[0], 0.0, (0, 0), 1))        # nothing but NaN: no hit, se = 4
    rows.append((np.array([0.7, 0.1, 0.1, 0.05, 0.05, 0, 0], np.float32), 0.0, np.eye(7, dtype=np.float32)[1], 0.0, full_columns([0]), 1))      # the largest p sits on a full column
    rows.append((np.array([0.7, 0.1, 0.1, 0.05, 0.05, 0, 0], np.float32), 0.0, np.eye(7, dtype=np.float32)[0], 0.0, full_columns([0]), 1))      # ... which the target names: no hit
    rows.append((np.array([0.3, 0.3, 0.1, 0.1, 0.1, 0.05, 0.05], np.float32), 0.0, np.array([0, 0.4, 0.4, 0.2, 0, 0, 0], np.float32), 0.0, (0, 0), 1))   # ties: lowest index on both sides
    rows.append((np.array([0.3, 0.3, 0.1, 0.1, 0.1, 0.05, 0.05], np.float32), 0.0, np.array([0.4, 0.4, 0, 0.2, 0, 0, 0], np.float32), 0.0, (0, 0), 1))
    rows.append((u, 1.0, u, -1.0, full_columns(range(7)), 1))                                               # a full board: no legal move, se = 4
    rows.append((u, 0.125, u, 0.25, (0, 0), 0))                                                             # weight 0
    p, v, pis, zs, states, w = (np.array([r[i] for r in rows], dt) for i, dt in enumerate((np.float32, np.float32, np.float32, np.float32, np.uint64, np.uint32)))
    got, want = tw.score(p, v, pis, zs, states, w), tw.score_py(p, v, pis, zs, states, w)
    assert_same_score(got, want)
    # by the rule: rows 1 and 10 have t* = m* = 0 (all ties), row 5's m* is the first legal maximum, row 8 ties at the lowest index on both sides
    assert [int(h) for h in got["hit"]] == [0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1]
    assert got["ce"][1] == 0 and got["kl"][1] == 0 and not np.signbit(got["ce"][1])
    assert got["se"][4] == 4 and got["se"][9] == 4 and np.isfinite(got["ce"]).all() and got["ce"].max() <= 128
    assert abs(got["ce"][0] - np.log(7)) < 1e-5
    # the floor: log2(2^-126) = -126 exactly for every p at or below it
    assert abs(got["ce"][2] - (4 * 126 * np.log(2) - np.log(0.5) - 2 * np.log(0.25)) / 7) < 1e-3
    # one tuple of weight 2^24 fills the window's whole weight: the sums are 2^24 times its K
    one = tw.score(p[:1], v[:1], pis[:1], zs[:1], states[:1], np.array([1 << 24], np.uint32))
    base = tw.score(p[:1], v[:1], pis[:1], zs[:1], states[:1])
    assert one["sums"] == tuple((1 << 24) * x for x in base["sums"]) and one["sums"][0] < 1 << 62
    assert one["sums"] == tw.score_py(p[:1], v[:1], pis[:1], zs[:1], states[:1], np.array([1 << 24], np.uint32))["sums"]
    assert tw.results(one["sums"]) == tw.results(base["sums"])


def test_holdout_rule():
    states = tw.random_states(4096, 11, distinct=True)
    n, P = len(states), 0.25
    for seed in (0, 7, 2 ** 63 + 5):
        held, keys = tw.holdout(states, P, seed)
        assert np.array_equal(held, tw.holdout_py(states, P, seed))
        assert np.array_equal(keys, np.array([tw.holdout_key_py(int(a), int(b)) for a, b in states], np.uint64))
        # a position and its mirror image are on one side
        mheld, mkeys = tw.holdout(tw.mirror_states(states), P, seed)
        assert np.array_equal(mheld, held) and np.array_equal(mkeys, keys)
        # the share: a binomial count within five standard deviations
        assert abs(int(held.sum()) - n * P) <= 5 * np.sqrt(n * P * (1 - P)), int(held.sum())
        assert not tw.holdout(states, 0.0, seed)[0].any() and tw.holdout(states, 1.0, seed)[0].all()
    assert not np.array_equal(tw.holdout(states, P, 0)[0], tw.holdout(states, P, 1)[0])
    # the split is nested in the share: what is held at 0.1 stays held at 0.25
    assert not (tw.holdout(states, 0.1, 3)[0] & ~tw.holdout(states, 0.25, 3)[0]).any()


def test_best_stop_rule():
    def hist(sums):
        return np.array([[s * 0.75, s * 0.25, 0.0, 0.0] for s in sums], np.float64)

    cases = [([1.0, 2.0, 3.0, 4.0], 0),            # the best epoch first
             ([3.0, 2.0, 1.0, 2.0, 3.0], 2),       # in the middle
             ([4.0, 3.0, 2.0, 1.0], 3),            # last
             ([2.0, 1.0, 1.0, 1.0], 1),            # ties: the first
             ([2.0, 2.0], 0), ([5.0], 0)]
    for sums, best in cases:
        for patience in (0, 1, 3):
            for n in range(1, len(sums) + 1):
                h = hist(sums[:n])
                got, want = tw.best_stop(h, patience), tw.best_stop_py(h, patience)
                assert got == want, (sums, patience, n)
            assert got[0] == best
    assert tw.best_stop(hist([1.0, 2.0, 3.0, 4.0]), 1) == (0, True) and tw.best_stop(hist([1.0, 2.0]), 1) == (0, True)
    assert tw.best_stop(hist([1.0, 2.0, 3.0]), 3) == (0, False) and tw.best_stop(hist([1.0, 2.0, 3.0, 4.0]), 3) == (0, True)
    assert tw.best_stop(hist([3.0, 2.0, 1.0, 2.0]), 1) == (2, True) and tw.best_stop(hist([3.0, 2.0, 1.0]), 1) == (2, False)
    assert tw.best_stop(hist([2.0, 1.0, 1.0]), 1) == (1, True)          # a tie is no new best
    assert tw.best_stop(hist([1.0, 2.0, 3.0, 4.0]), 0) == (0, False)    # patience off never stops
    nan = hist([float("nan"), 2.0, float("nan")])
    assert tw.best_stop(nan, 1) == tw.best_stop_py(nan, 1) == (1, True)


def test_the_library_exports_the_new_symbols(engine_mod):
    lib = ctypes.CDLL(engine_mod.LIB_PATH)
    for name in ("az_net_evaluate", "az_samples_holdout", "az_net_train_set_validation", "az_net_train_validation"):
        assert hasattr(lib, name) and name in engine_mod.EXPORTS
    for name in ("evaluate", "samples_holdout", "train_set_validation", "train_validation"):
        assert callable(getattr(engine_mod.Engine, name))


def test_python_coach_split_partitions_the_window(engine_mod, oracle, tmp_path):
    """validation_share on a fake engine: the trained part and the registered part partition the window by the rule, the history and the
    .examples files keep every tuple, and the report carries the new keys."""
    from alphazero_rs_amd import coach
    from net_ref import random_params
    from test_coach_cpu import FakeEngine

    def states_of(boards):
        b = np.asarray(boards).reshape(-1, 2, 6, 7)
        s = np.zeros((len(b), 2), np.uint64)
        for r in range(6):
            for c in range(7):
                bit = np.uint64(1) << np.uint64(c * 7 + (5 - r))
                for pl in range(2):
                    s[:, pl] |= np.where(b[:, pl, r, c] != 0, bit, np.uint64(0))
        return s

    class Fake(FakeEngine):
        def __init__(self, *a):
            super().__init__(*a)
            self.options, self.trained, self.val, self.cleared = {}, [], [], 0

        def set_option(self, key, value):
            self.options[key] = value

        def samples_holdout(self, share, seed, pis, zs, *, states=None, boards=None):
            return tw.holdout_py(states_of(boards), share, seed)

        def train_set_validation(self, pis=None, zs=None, *, states=None, boards=None, weights=None):
            if pis is None:
                self.cleared += 1
            else:
                self.val.append((boards.copy(), pis.copy(), zs.copy(), dict(self.options)))

        def train(self, prev_id, model_id, boards, pis, vs):
            self.trained.append((boards.copy(), pis.copy(), vs.copy(), dict(self.options)))
            self.params[model_id] = self.params[prev_id] + np.float32(1e-3)
            return [(1.0, 0.5)]

        def train_validation(self):
            return [(0.9, 0.4, 0.1, 0.5), (0.8, 0.3, 0.1, 0.6)], 1

    def run(d, share):
        eng = Fake(oracle, 16)
        eng.net_set_params(0, random_params(16, 9, bn_random=False))
        c = coach.Coach.setup(eng, d, 1000000, 0.6, 15, 2, 10000, 1, 64, 6, 2, 5, 10, 1, 1000, 1, log=lambda m: None)
        c.validation_share, c.keep_best, c.patience = share, share > 0, 2 if share > 0 else 0
        return c, eng, c.learn(seed=4)

    c, eng, rep = run(os.path.join(tmp_path, "val"), 0.25)
    c0, eng0, rep0 = run(os.path.join(tmp_path, "plain"), 0.0)
    assert len(eng.trained) == len(eng.val) == 2 and eng.cleared == 2 and not eng0.val and eng0.cleared == 0
    key = lambda b, p, z: sorted(zip(map(bytes, np.ascontiguousarray(b).reshape(len(z), -1)), map(bytes, np.ascontiguousarray(p)), map(float, z)))
    for it in range(2):
        tb, tp, tz, topt = eng.trained[it]
        vb, vp, vz, _ = eng.val[it]
        wb, wp, wz, _ = eng0.trained[it] if it == 0 else (None,) * 4
        assert rep[it]["val_n"] == len(vz) > 0 and rep[it]["samples"] == len(tz) and rep[it]["samples_raw"] == len(tz) + len(vz)
        assert topt["train_keep_best"] == 1 and topt["train_patience"] == 2
        assert tw.holdout_py(states_of(vb), 0.25, 4).all() and not tw.holdout_py(states_of(tb), 0.25, 4).any()
        if it == 0:            # the same episodes as the plain run: the two parts are its window, tuple for tuple
            assert key(np.concatenate([tb, vb]), np.concatenate([tp, vp]), np.concatenate([tz, vz])) == key(wb, wp, wz)
        assert rep[it]["val_loss_pi"] == [0.9, 0.8] and rep[it]["val_loss_v"] == [0.4, 0.3] and rep[it]["val_top1"] == [0.5, 0.6]
        assert rep[it]["best_epoch"] == 1
    assert eng.options == {"train_seed": 5, "train_keep_best": 0, "train_patience": 0}
    assert "val_n" not in rep0[0] and "best_epoch" not in rep0[0]
    # history is not split: the first iteration's file is the plain run's, byte for byte
    with open(os.path.join(tmp_path, "val", "0.examples"), "rb") as x, open(os.path.join(tmp_path, "plain", "0.examples"), "rb") as y:
        assert x.read() == y.read()
    assert sum(h[2].shape[0] for h in c.history) == rep[1]["samples_raw"]
    c.validation_share, c.keep_best = 0.0, True
    with pytest.raises(ValueError):
        c.learn(seed=4)
