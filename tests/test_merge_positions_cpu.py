"""Position averaging without a GPU (az_samples_merge): the numpy twin against a hand computation, the associativity
the contract rests on, the bindings, and the Coach with the feature off and on (stub engine, stub trainer)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import merge_twin as mg
import mirror_twin as mt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = (0, 0)
CENTRE = (0, 1 << 21)                 # one stone of the other side in column 3: its own mirror image
LEFT, RIGHT = (0, 1 << 0), (0, 1 << 42)      # a stone in column 0 / column 6: mirror images of each other; LEFT packs to the smaller word


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def hand_case():
    """[EMPTY, CENTRE, LEFT, EMPTY, RIGHT, EMPTY]: three copies of one position with different pi, a singleton with a denormal pi
    entry, a mirrored pair."""
    states = np.array([EMPTY, CENTRE, LEFT, EMPTY, RIGHT, EMPTY], np.uint64)
    pis = np.zeros((6, 7), np.float32)
    pis[0, 0] = pis[3, 1] = pis[5, 2] = 1.0                                  # the three copies: one-hot on columns 0, 1, 2
    pis[1] = [0, 0.5, 0, 0.25, 0, 0.25, 0]
    pis[1, 0] = np.array([1], np.uint32).view(np.float32)[0]                 # the smallest denormal, bits 0x00000001
    pis[2] = [0.5, 0.25, 0, 0, 0, 0, 0.25]
    pis[4] = [0, 0, 0, 0, 0, 0.5, 0.5]
    zs = np.array([1, 0.5, 1, -1, -1, mg.DRAW_EPS], np.float32)
    return states, pis, zs


def test_twin_against_a_hand_computation():
    states, pis, zs = hand_case()
    third = 0x3EAAAAAB                                 # 1/3 to the nearest f32
    # z of the triple: (2^38 - 2^38 + 27487790) / (3 * 2^38); 1e-4f = 13743895 * 2^-37 exactly, so q(DRAW_EPS) = 27487790
    assert bits(mg.DRAW_EPS) == 0x38D1B717 and int(mg.quantise(mg.DRAW_EPS)) == 27487790
    z3 = 0x380BCF65
    exact = Fraction(27487790, 3 * 2 ** 38)
    z3f = np.array([z3], np.uint32).view(np.float32)[0]
    for nb in (np.nextafter(z3f, np.float32(0)), np.nextafter(z3f, np.float32(1))):
        assert abs(Fraction(float(z3f)) - exact) < abs(Fraction(float(nb)) - exact)
    got = mg.merge(pis, zs, states=states)
    assert got["count"] == 4 and got["counts"].tolist() == [3, 1, 1, 1]
    assert got["states"].tolist() == [list(EMPTY), list(CENTRE), list(LEFT), list(RIGHT)]        # first-occurrence order
    assert bits(got["pis"][0]).tolist() == [third, third, third, 0, 0, 0, 0] and bits(got["zs"][0]) == z3
    # the singleton is verbatim: its denormal survives, where the mean path would have quantised it to 0
    assert bits(got["pis"][1]).tolist() == bits(pis[1]).tolist() and bits(got["pis"][1])[0] == 1 and int(mg.quantise(pis[1, 0])) == 0
    assert bits(got["zs"][1]) == bits(np.float32(0.5))
    assert np.array_equal(bits(got["pis"][2:]), bits(pis[[2, 4]])) and np.array_equal(bits(got["zs"][2:]), bits(zs[[2, 4]]))
    assert np.array_equal(got["boards"], mt.states_to_boards(got["states"])) and got["boards"].sum() == 3
    # canonical: LEFT and RIGHT merge under LEFT, RIGHT's pi reversed: ([.5, .25, 0, 0, 0, 0, .25] + [.5, .5, 0, 0, 0, 0, 0]) / 2
    can = mg.merge(pis, zs, states=states, canonical=True)
    assert can["count"] == 3 and can["counts"].tolist() == [3, 1, 2]
    assert can["states"].tolist() == [list(EMPTY), list(CENTRE), list(LEFT)]
    assert np.array_equal(bits(can["pis"][:2]), bits(got["pis"][:2]))
    assert can["pis"][2].tolist() == [0.5, 0.375, 0, 0, 0, 0, 0.125] and bits(can["zs"][2]) == 0
    # a mirrored singleton is canonicalised, which is exact
    one = mg.merge(pis[4:5], zs[4:5], states=states[4:5], canonical=True)
    assert one["states"].tolist() == [list(LEFT)] and np.array_equal(bits(one["pis"][0]), bits(pis[4, ::-1])) and bits(one["zs"]) == bits(zs[4])
    # the boards route is the states route
    viab = mg.merge(pis, zs, boards=mt.states_to_boards(states), canonical=True)
    for k in can:
        assert np.array_equal(viab[k], can[k]), k
    assert mg.merge(pis[:0], zs[:0], states=states[:0])["count"] == 0


def test_twin_refusals():
    states, pis, zs = hand_case()
    ok = dict(states=states)
    assert mg.refusal(pis, zs, **ok) is None and mg.refusal(pis, zs, boards=mt.states_to_boards(states)) is None

    def changed(a, idx, v):
        a = a.copy()
        a[idx] = v
        return a
    assert mg.refusal(changed(pis, (2, 3), 1.5), zs, **ok) and mg.refusal(pis, changed(zs, 1, -2), **ok)
    assert mg.refusal(changed(pis, (0, 0), np.nan), zs, **ok) == "NaN" and mg.refusal(pis, changed(zs, 0, np.nan), **ok) == "NaN"
    assert mg.refusal(pis, zs, states=changed(states, (1, 0), 1 << 21)) == "overlapping stones"
    assert mg.refusal(pis, zs, states=changed(states, (0, 0), 1 << 6)) == "bits outside the board"
    assert mg.refusal(pis, zs, states=changed(states, (0, 1), 1 << 49)) == "bits outside the board"
    b = mt.states_to_boards(states)
    assert mg.refusal(pis, zs, boards=changed(b, (0, 0, 5, 0), 0.5)) == "feature not 0 or 1"
    assert mg.refusal(pis, zs, boards=changed(b, (1, 0, 5, 3), 1.0)) == "both planes set"
    assert mg.refusal(pis, zs, capacity=5, **ok) == "capacity < n" and mg.refusal(pis, zs, capacity=6, **ok) is None
    assert mg.refusal(pis, zs, flags=2, **ok) == "unknown flag bits" and mg.refusal(pis, zs, flags=1, **ok) is None


def test_integer_sums_do_not_depend_on_the_order():
    rng = np.random.default_rng(5)
    x = (rng.random(100000).astype(np.float32) * 2 - 1)
    x[:4] = [1.0, -1.0, mg.DRAW_EPS, -mg.DRAW_EPS]
    q = mg.quantise(x)
    assert np.abs(q).max() <= 2 ** 38
    total = int(q.sum(dtype=np.int64))
    assert total == sum(int(v) for v in q)                       # no wrap
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(len(q))
        assert int(q[p].sum(dtype=np.int64)) == total
        assert int(np.add.reduce(q[p].reshape(100, -1).sum(axis=1, dtype=np.int64))) == total     # combined in blocks first
    # the stated bound: 2^24 copies of +1 or -1 stay inside int64, and their mean is exactly +-1
    for v in (1.0, -1.0):
        s = np.broadcast_to(mg.quantise(v), (mg.MAX_TUPLES,)).sum(dtype=np.int64)
        assert int(s) == int(v) * 2 ** 62 and abs(int(s)) < 2 ** 63
        assert mg.mean_of(s, mg.MAX_TUPLES) == np.float32(v)


def test_bindings_carry_the_export(engine_mod):
    assert "az_samples_merge" in engine_mod.EXPORTS and engine_mod.MERGE_CANONICAL == 1
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "az_engine.h")).read(), flags=re.S)
    args = re.search(r"az_status\s+az_samples_merge\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")
    assert len(args) == 5 and not any(re.search(r"\bin$", a.strip()) for a in args)
    assert re.search(r"#define\s+AZ_MERGE_CANONICAL\s+1\b", hdr)
    fn = engine_mod._lib.az_samples_merge
    assert len(fn.argtypes) == len(args) and fn.restype is engine_mod.C.c_int32
    assert hasattr(engine_mod.Engine, "merge_samples")


# ---- the Coach -----------------------------------------------------------------------------------------------------------------------------
class StubEngine:
    """Ten short episodes that all walk the same first plies: plenty of duplicates.  merge_samples is the twin, or forbidden."""

    def __init__(self, allow_merge):
        self.allow_merge, self.params, self.merge_calls = allow_merge, {0: np.zeros(4, np.float32)}, []

    def net_save(self, model_id, path):
        self.params[model_id].tofile(path)

    def net_get_params(self, model_id):
        return self.params[model_id].copy()

    def net_set_params(self, model_id, p):
        self.params[model_id] = np.asarray(p, np.float32).copy()

    def selfplay(self, n_games, **kw):
        rng = np.random.default_rng(kw["seed"] + kw["first_game_id"])
        states, s = [], (0, 0)
        for g in range(n_games):
            s = (0, 0)
            for ply in range(4):
                states.append(s)
                a = [3, 3, 2, g % 7][ply]
                mask = s[0] | s[1]
                s = (s[1], s[0] | ((mask + (1 << (a * 7))) & (0x3F << (a * 7))))
        n = len(states)
        pis, zs = mg.random_targets(rng, n)
        return {"states": np.array(states, np.uint64), "pis": pis, "zs": zs, "count": n}

    def arena(self, num_games, num_sims, **kw):
        return np.array([num_games, 0, 0], np.uint64), np.ones(num_games, np.int8)

    def merge_samples(self, pis, zs, *, states=None, boards=None, canonical=False, want_boards=False):
        if not self.allow_merge:
            raise AssertionError("merge_samples called with merge_positions off")
        self.merge_calls.append((np.array(boards), np.array(pis), np.array(zs), canonical, want_boards, states))
        return mg.merge(pis, zs, boards=boards, canonical=canonical)


class StubTrainer:
    def __init__(self):
        self.seen, self.history = [], [(0.0, 0.0)]

    def train(self, prev, boards, pis, vs, seed=0):
        self.seen.append((np.array(boards), np.array(pis), np.array(vs)))
        return prev + 1


def run_coach(tmp, **fields):
    from alphazero_rs_amd import coach
    eng, tr = StubEngine(allow_merge=bool(fields.get("merge_positions"))), StubTrainer()
    c = coach.Coach.setup(eng, tmp, 1000000, 0.6, 15, 3, 100000, 1, 64, 4, 1, 10, 10, 1, 1000, 1, trainer=tr, log=lambda m: None)
    assert c.merge_positions is False and c.merge_canonical is False             # the defaults
    for k, v in fields.items():
        setattr(c, k, v)
    return c, eng, tr, c.learn(seed=7)


def test_coach_never_asks_with_the_feature_off(engine_mod, tmp_path):
    c, eng, tr, rep = run_coach(str(tmp_path))
    assert eng.merge_calls == [] and rep[0]["samples"] == rep[0]["samples_raw"] == 80 == len(tr.seen[0][2])


@pytest.mark.parametrize("canonical", [False, True])
def test_coach_trains_on_the_merged_then_shuffled_set(engine_mod, tmp_path, canonical):
    from alphazero_rs_amd import coach
    c, eng, tr, rep = run_coach(str(tmp_path / "on"), merge_positions=True, merge_canonical=canonical)
    _, _, _, rep_off = run_coach(str(tmp_path / "off"))
    assert len(eng.merge_calls) == 1
    boards, pis, zs, flag, want_boards, states = eng.merge_calls[0]
    assert flag is canonical and want_boards is True and states is None
    # the engine was handed the raw window: what history holds and 0.examples stores
    hb, hp, hz = c.history[0]
    assert np.array_equal(boards, hb) and np.array_equal(pis, hp) and np.array_equal(zs, hz) and len(hz) == 80
    want = mg.merge(hp, hz, boards=hb, canonical=canonical)
    m = want["count"]
    assert 0 < m < 80 and rep[0]["samples"] == m and rep[0]["samples_raw"] == 80
    perm = coach.shuffle_permutation(m, 7, 0)
    tb, tp, tz = tr.seen[0]
    assert np.array_equal(tb, want["boards"][perm]) and np.array_equal(bits(tp), bits(want["pis"][perm])) and np.array_equal(bits(tz), bits(want["zs"][perm]))
    # history and the examples file stay raw: byte for byte the feature-off run's
    with open(tmp_path / "on" / "0.examples", "rb") as a, open(tmp_path / "off" / "0.examples", "rb") as b:
        assert a.read() == b.read()
    assert sorted(set(rep[0]) - set(rep_off[0])) == [] and rep_off[0]["samples"] == 80
    if canonical:
        assert m < mg.merge(hp, hz, boards=hb)["count"]              # the stub's last plies come in mirrored pairs
