"""The window check of csrc/az_samples.h without a GPU: its g++ build (tests/samples_twin.py) against independent numpy restatements --
merge_twin.refusal for the [-1, 1] route, mirror_twin.boards_to_states for the planes, a [0, 1] variant written here -- on a window of 300
tuples with one fault at a time; the refusal sentences as literals; and the header compiled alone by g++ with AddressSanitizer and UBSan,
run as a stand-alone program (tests/cpp/samples_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import merge_twin
import mirror_twin
import samples_twin as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300
PLACES = (0, 255, 256, 299)
V, S, F, P = st.BAD_VALUE, st.BAD_STATE, st.BAD_FEATURE, st.BAD_PRIOR

FEATURE_TEXT = "a boards feature that is not 0 or 1, or a cell set in both planes"
STATE_TEXT = "a state with overlapping stones or bits outside the 7x6 board"
VALUE_TEXT = "a pi or z that is NaN or outside [-1, 1]"
VALUE_TEXT_STRICT = "a pi that is NaN or outside [0, 1], or a z that is NaN or outside [-1, 1]"
PRIOR_TEXT = "a prior that is NaN or outside [0, 1]"

# name -> (route it applies to (None: both), bits where pi may be in [-1, 1], bits where pi must be in [0, 1])
FAULTS = {
    "nan_pi": (None, V, V),
    "pi_1.5": (None, V, V),
    "pi_-0.5": (None, 0, V),
    "z_-1.5": (None, V, V),
    "nan_z": (None, V, V),
    "stones_twice": ("states", S, S),
    "column_bit_6": ("states", S, S),
    "feature_0.5": ("boards", F, F),
    # a cell set in both planes is a stone of both sides in the state rebuilt from them: the feature bit and the state bit
    "both_planes": ("boards", F | S, F | S),
}


@pytest.fixture(scope="module")
def window():
    rng = np.random.default_rng(20)
    states = merge_twin.random_positions(rng, N)
    pis, zs = merge_twin.random_targets(rng, N)
    w = {"states": states, "boards": mirror_twin.states_to_boards(states).reshape(N, 84), "pis": pis, "zs": zs}
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
        w["boards"][at, 5 * 7 + 3] = 0.5
    elif name == "both_planes":
        w["boards"][at, 5 * 7 + 3] = w["boards"][at, 42 + 5 * 7 + 3] = 1.0
    else:
        raise KeyError(name)
    return w


REASON_BIT = {"NaN": V, "value outside [-1, 1]": V, "feature not 0 or 1": F, "both planes set": F, "overlapping stones": S, "bits outside the board": S}


def refusal_np(w, route, strict):
    """The reason the numpy restatement gives, as its verdict bit (0: the window is legal)."""
    with np.errstate(invalid="ignore"):
        if strict and not np.isnan(w["pis"]).any() and (w["pis"] < 0).any():
            return V
    why = merge_twin.refusal(w["pis"], w["zs"], **{route: w[route]})
    return 0 if why is None else REASON_BIT[why]


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("route", ["states", "boards"])
def test_clean_window(window, route, strict):
    word, bits, seen = st.check(window["pis"], window["zs"], strict_pi=strict, **{route: window[route]})
    assert word == 0 and not bits.any() and refusal_np(window, route, strict) == 0
    assert np.array_equal(seen, window["states"])
    if route == "boards":
        assert np.array_equal(seen, mirror_twin.boards_to_states(window["boards"]))


@pytest.mark.parametrize("at", PLACES)
@pytest.mark.parametrize("name", sorted(FAULTS))
def test_one_fault(window, name, at):
    only, loose, tight = FAULTS[name]
    w = with_fault(window, name, at)
    for route in ("states", "boards"):
        if only not in (None, route):
            continue
        for strict, want in ((False, loose), (True, tight)):
            word, bits, _ = st.check(w["pis"], w["zs"], strict_pi=strict, **{route: w[route]})
            expect = np.zeros(N, np.uint32)
            expect[at] = want
            assert word == want and np.array_equal(bits, expect), (route, strict, word)
            ref = refusal_np(w, route, strict)
            assert (ref == 0) == (want == 0) and ref & want == ref, (route, strict, ref)


def test_bad_text_literals():
    for strict in (False, True):
        value = VALUE_TEXT_STRICT if strict else VALUE_TEXT
        assert st.bad_text(0, strict) is None
        assert st.bad_text(V, strict) == value
        assert st.bad_text(S, strict) == STATE_TEXT
        assert st.bad_text(F, strict) == FEATURE_TEXT
        assert st.bad_text(P, strict) == PRIOR_TEXT
        # feature, then state, then value, then prior
        assert st.bad_text(F | S, strict) == FEATURE_TEXT
        assert st.bad_text(F | V, strict) == FEATURE_TEXT
        assert st.bad_text(S | V, strict) == STATE_TEXT
        assert st.bad_text(S | P, strict) == STATE_TEXT
        assert st.bad_text(V | P, strict) == value
        assert st.bad_text(F | S | V | P, strict) == FEATURE_TEXT


def test_header_alone_under_sanitizers(tmp_path):
    """csrc/az_samples.h needs nothing of HIP: g++ compiles it alone, and the stand-alone program runs clean under ASan + UBSan."""
    exe = os.path.join(tmp_path, "samples_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "samples_check.cpp"), "-o", exe])
    assert subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip() == "ok"
