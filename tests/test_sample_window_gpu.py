"""What the five entries that check a window of training tuples refuse, and with which words (az_samples_merge, az_samples_surprise,
az_net_evaluate, az_samples_holdout, az_net_train_set_validation; include/az_engine.h, csrc/az_samples.h): one fault at a time at the
edges of the 256-tuple workgroups, on the states and the boards route, with the status, the exact az_last_error text and untouched
outputs; then the clean window through the same calls against the twins, bit for bit.

One engine with net_channels = 128 and max_batch = 64, a random-init model, 300 tuples: two workgroups of 256 with a partial second one,
five forward chunks with a partial last one.  Nothing here depends on how the engine arrives at a refusal: every sentence is a literal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                   # noqa: F401  before the engine library is loaded: torch brings its own HIP runtime, and a process wants one

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import merge_twin              # noqa: E402
import mirror_twin             # noqa: E402
import score_twin              # noqa: E402
import target_twin             # noqa: E402

N, MODEL = 300, 3
PLACES = (0, 255, 256, 299)
BAD_ARGUMENT = 1
SHARE, SEED = 0.5, 11

FEATURE = "a boards feature that is not 0 or 1, or a cell set in both planes"
STATE = "a state with overlapping stones or bits outside the 7x6 board"
VALUE = "a pi or z that is NaN or outside [-1, 1]"
VALUE_STRICT = "a pi that is NaN or outside [0, 1], or a z that is NaN or outside [-1, 1]"
ENTRIES = {"merge": "az_samples_merge", "surprise": "az_samples_surprise", "evaluate": "az_net_evaluate", "holdout": "az_samples_holdout",
           "set_validation": "az_net_train_set_validation"}
STRICT = ("evaluate", "set_validation")              # a pi below 0 is refused
# name -> (the route it exists on (None: both), what it is: "value", "pi<0", "state" or "feature")
FAULTS = {"nan_pi": (None, "value"), "pi_1.5": (None, "value"), "pi_-0.5": (None, "pi<0"), "z_-1.5": (None, "value"), "nan_z": (None, "value"),
          "stones_twice": ("states", "state"), "column_bit_6": ("states", "state"), "feature_0.5": ("boards", "feature"),
          "both_planes": ("boards", "feature")}


def sentence(entry, kind):
    """The refusal of `kind` by `entry`, or None where the entry accepts it."""
    if kind == "pi<0" and entry not in STRICT:
        return None
    text = {"value": VALUE_STRICT if entry in STRICT else VALUE, "pi<0": VALUE_STRICT, "state": STATE, "feature": FEATURE}[kind]
    return ENTRIES[entry] + ": " + text


@pytest.fixture(scope="module")
def wengine(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=64, net_channels=128)
    e.net_init_random(MODEL, seed=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def window():
    """300 tuples over 200 distinct positions, so that az_samples_merge has copies to average."""
    rng = np.random.default_rng(21)
    states = merge_twin.random_positions(rng, 200)[rng.integers(0, 200, N)]
    pis, zs = merge_twin.random_targets(rng, N)
    priors = rng.dirichlet(np.ones(7), N).astype(np.float32)
    w = {"states": np.ascontiguousarray(states), "boards": np.ascontiguousarray(mirror_twin.states_to_boards(states)), "pis": pis, "zs": zs,
         "priors": priors}
    for a in w.values():
        a.setflags(write=False)
    return w


def with_fault(window, name, at):
    w = {k: v.copy() for k, v in window.items()}
    if name == "nan_pi":
        w["pis"][at, 2] = np.nan
    elif name == "pi_1.5":
        w["pis"][at, 6] = 1.5
    elif name == "pi_-0.5":
        w["pis"][at, 0] = -0.5
    elif name == "z_-1.5":
        w["zs"][at] = -1.5
    elif name == "nan_z":
        w["zs"][at] = np.nan
    elif name == "stones_twice":
        w["states"][at] |= np.uint64(1 << 21)                       # the bottom cell of column 3, for both sides
    elif name == "column_bit_6":
        w["states"][at, 1] |= np.uint64(1 << (4 * 7 + 6))
    elif name == "feature_0.5":
        w["boards"][at, 0, 5, 3] = 0.5
    elif name == "both_planes":
        w["boards"][at, 0, 5, 3] = w["boards"][at, 1, 5, 3] = 1.0
    else:
        raise KeyError(name)
    return w


class Outputs:
    """Every array an entry could write, filled with a sentinel."""

    def __init__(self):
        cap = 2 * N
        self.a = {"states": np.full((cap, 2), 9, np.uint64), "boards": np.full((cap, 2, 6, 7), 7.0, np.float32), "pis": np.full((cap, 7), 7.0, np.float32),
                  "zs": np.full(cap, 7.0, np.float32), "counts": np.full(cap, 9, np.uint32), "kl": np.full(N, 7.0, np.float32),
                  "ce": np.full(N, 7.0, np.float32), "se": np.full(N, 7.0, np.float32), "score": np.full(6, 7.0, np.float64),
                  "sums": np.full(5, 9, np.uint64), "held": np.full(N, 9, np.uint8)}

    def untouched(self):
        return all(np.all(v == (9 if v.dtype.kind == "u" else 7.0)) for v in self.a.values())


def call(e, em, entry, w, route, out):
    """(status, az_last_error, dst count) of one raw call on one route; the outputs go to `out`."""
    lib, h, ptr, o = e._lib, e._h, em._ptr, out.a
    st, bd = (w["states"], None) if route == "states" else (None, w["boards"])
    src = em.az_samples(N, N, ptr(st), ptr(bd), ptr(w["pis"]), ptr(w["zs"]), None, None)
    dst = em.az_samples(2 * N, 0, ptr(o["states"]) if st is not None else None, ptr(o["boards"]) if bd is not None else None, ptr(o["pis"]), ptr(o["zs"]),
                        None, None)
    if entry == "merge":
        status = lib.az_samples_merge(h, C.byref(src), 0, C.byref(dst), ptr(o["counts"]))
    elif entry == "surprise":
        status = lib.az_samples_surprise(h, C.byref(src), ptr(w["priors"]), int(SHARE * 1e6), SEED, C.byref(dst), ptr(o["counts"]), ptr(o["kl"]))
    elif entry == "evaluate":
        status = lib.az_net_evaluate(h, MODEL, C.byref(src), None, ptr(o["score"]), ptr(o["sums"]), ptr(o["ce"]), ptr(o["se"]), ptr(o["kl"]))
    elif entry == "holdout":
        status = lib.az_samples_holdout(h, C.byref(src), int(SHARE * 1e6), SEED, ptr(o["held"]))
    elif entry == "set_validation":
        status = lib.az_net_train_set_validation(h, C.byref(src), None)
    else:
        raise KeyError(entry)
    return status, lib.az_last_error(h).decode(), int(dst.count)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check_clean(e, em, entry, window, route):
    """The clean window through `entry`: accepted, and equal to the twin bit for bit."""
    out = Outputs()
    status, text, count = call(e, em, entry, window, route, out)
    assert status == 0, (entry, route, text)
    o, states, pis, zs = out.a, window["states"], window["pis"], window["zs"]
    if entry == "merge":
        want = merge_twin.merge(pis, zs, states=states)
        m = want["count"]
        assert count == m < N
        assert np.array_equal(bits(o["pis"][:m]), bits(want["pis"])) and np.array_equal(bits(o["zs"][:m]), bits(want["zs"]))
        assert np.array_equal(o["counts"][:m], want["counts"]) and np.all(o["counts"][m:] == 9)
        if route == "states":
            assert np.array_equal(o["states"][:m], want["states"])
        else:
            assert np.array_equal(bits(o["boards"][:m]), bits(want["boards"]))
    elif entry == "surprise":
        want = target_twin.surprise(pis, window["priors"], SHARE, SEED)
        x_states, x_boards, x_pis, x_zs = target_twin.expand(want["counts"], states, window["boards"], pis, zs)
        m = int(want["total"])
        assert count == m and np.array_equal(o["counts"][:N], want["counts"]) and np.array_equal(bits(o["kl"]), bits(want["kl"]))
        assert np.array_equal(bits(o["pis"][:m]), bits(x_pis)) and np.array_equal(bits(o["zs"][:m]), bits(x_zs))
        if route == "states":
            assert np.array_equal(o["states"][:m], x_states)
        else:
            assert np.array_equal(bits(o["boards"][:m]), bits(x_boards))
    elif entry == "evaluate":
        p, v = e.predict_states(states, MODEL)
        want = score_twin.score_py(p, v, pis, zs, states)
        assert tuple(int(x) for x in o["sums"]) == tuple(want["sums"])
        assert tuple(o["score"]) == (float(N), float(N)) + score_twin.results(want["sums"])
        for got, key in ((o["ce"], "ce"), (o["se"], "se"), (o["kl"], "kl")):
            assert np.array_equal(bits(got), bits(want[key])), key
    elif entry == "holdout":
        assert np.array_equal(o["held"].astype(bool), score_twin.holdout_py(states, SHARE, SEED))
    elif entry == "set_validation":
        assert e.train_validation() == ([], -1)
        e.train_set_validation()                         # cleared again: the engine is left as it was found


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_one_fault_at_a_time(wengine, engine_mod, window, entry):
    e = wengine
    out = Outputs()
    for name, (only, kind) in FAULTS.items():
        want = sentence(entry, kind)
        for at in PLACES:
            w = with_fault(window, name, at)
            for route in ("states", "boards"):
                if only not in (None, route):
                    continue
                status, text, _ = call(e, engine_mod, entry, w, route, out if want else Outputs())
                print(entry, name, at, route, status, text if status else "")
                if want is None:
                    assert status == 0, (name, at, route, text)
                    if entry == "set_validation":
                        e.train_set_validation()
                else:
                    assert status == BAD_ARGUMENT and text == want, (name, at, route, status, text)
                    assert out.untouched(), (name, at, route)
    # two faults in one window: az_samples_holdout names the value, every other entry the state
    w = with_fault(with_fault(window, "z_-1.5", 299), "stones_twice", 0)
    status, text, _ = call(e, engine_mod, entry, w, "states", out)
    assert status == BAD_ARGUMENT and text == sentence(entry, "value" if entry == "holdout" else "state"), text
    assert out.untouched()
    # and behind all the refusals the clean window goes through and equals the twin
    for route in ("states", "boards"):
        check_clean(e, engine_mod, entry, window, route)
