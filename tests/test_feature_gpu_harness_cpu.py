"""The comparators of tests/feature_gpu.py compare what they claim to: each passes on equal data and raises on a change of any one field.
No GPU and no engine: the data is a small run of the twin (tests/selfplay_twin.py) and a stub that replays slices of it."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg        # noqa: E402
import selfplay_twin as tw      # noqa: E402


@pytest.fixture(scope="module")
def ref():
    """6 games of 8 simulations under a playout cap of 4 at P = 0.5: the masks are neither empty nor all-ones.  Left unchanged."""
    r = tw.selfplay(6, 8, cap_sims=4, full_e6=500000, net_kind=tw.NET_HASH, salt=fg.oracle_salt(10), seed=11, first_game_id=1000)
    full, plies = tw.popcount(r["full_masks"]), int(r["game_len"].sum())
    assert 0 < full < plies and r["count"] == 2 * full
    return r


def _as_engine(ref):
    """What run_selfplay would return for an engine that agrees with the twin"""
    got = {k: copy.deepcopy(ref[k]) for k in ("count", "game_len", "moves", "boards", "pis", "zs", "full_masks")}
    got["stats"] = {"simulations": ref["sims"], "samples": tw.popcount(ref["full_masks"]), "moves": int(ref["game_len"].sum()),
                    "games": len(ref["game_len"])}
    return got


def _bump(a, index):
    a[index] += 1


def _one_ulp(got):
    i = np.flatnonzero(got["pis"].reshape(-1))[0]
    got["pis"].reshape(-1).view(np.uint32)[i] += 1


def _flip_z(got):
    i = np.flatnonzero(got["zs"])[0]
    got["zs"][i] = -got["zs"][i]


ALTERATIONS = {
    "game_len": lambda g: _bump(g["game_len"], 3),
    "moves": lambda g: _bump(g["moves"], (2, 1)),
    "full_masks": lambda g: g["full_masks"].__setitem__(4, g["full_masks"][4] ^ np.uint64(1)),
    "count": lambda g: g.__setitem__("count", g["count"] + 2),
    "boards": lambda g: _bump(g["boards"].reshape(-1), 85),
    "pis": _one_ulp,
    "zs": _flip_z,
    "simulations": lambda g: _bump(g["stats"], "simulations"),
    "samples": lambda g: _bump(g["stats"], "samples"),
    "stats-moves": lambda g: _bump(g["stats"], "moves"),
    "games": lambda g: _bump(g["stats"], "games"),
}


def test_twin_comparator_passes_on_a_copy(ref):
    assert fg.check_samples_against_twin(_as_engine(ref), ref) == (tw.popcount(ref["full_masks"]), int(ref["game_len"].sum()))


@pytest.mark.parametrize("field", list(ALTERATIONS))
def test_twin_comparator_fails_on_one_altered_field(ref, field):
    got = _as_engine(ref)
    ALTERATIONS[field](got)
    with pytest.raises(AssertionError):
        fg.check_samples_against_twin(got, ref)


def test_tuple_comparator_without_symmetries(ref):
    """step 2: a run without symmetries holds every second tuple of the twin's"""
    got = _as_engine(ref)
    got.update(count=ref["count"] // 2, boards=ref["boards"][::2].copy(), pis=ref["pis"][::2].copy(), zs=ref["zs"][::2].copy())
    fg.check_tuples_against_twin(got, ref, step=2)
    with pytest.raises(AssertionError):
        fg.check_tuples_against_twin(got, ref)
    _one_ulp(got)
    with pytest.raises(AssertionError):
        fg.check_tuples_against_twin(got, ref, step=2)


# ---- the directory comparison ---------------------------------------------------------------------------------------------------------------
def _checkpoints(tmp_path, name, files):
    d = tmp_path / name
    d.mkdir()
    for f, data in files.items():
        (d / f).write_bytes(data)
    return str(d)


FILES = {"0.examples": b"examples" * 100, "0.aznet": b"w0", "1.aznet": b"w1" * 50, "coach.state": b"0 1\n"}


def test_directory_comparison_passes_on_equal_directories(tmp_path):
    a, b = _checkpoints(tmp_path, "a", FILES), _checkpoints(tmp_path, "b", FILES)
    assert fg.compare_directories(a, b) == sorted(FILES)


@pytest.mark.parametrize("case", ["one-byte", "missing-in-a", "missing-in-b", "no-examples", "no-candidate"])
def test_directory_comparison_fails(tmp_path, case):
    fa, fb = dict(FILES), dict(FILES)
    if case == "one-byte":
        fb["1.aznet"] = FILES["1.aznet"][:-1] + b"x"
    elif case == "missing-in-a":
        del fa["coach.state"]
    elif case == "missing-in-b":
        del fb["0.aznet"]
    elif case == "no-examples":
        del fa["0.examples"], fb["0.examples"]
    else:
        del fa["1.aznet"], fb["1.aznet"]
    with pytest.raises(AssertionError):
        fg.compare_directories(_checkpoints(tmp_path, "a", fa), _checkpoints(tmp_path, "b", fb))


# ---- the flatten and chunk helpers ------------------------------------------------------------------------------------------------------------
def test_flatten_eval_log():
    rng = np.random.default_rng(3)
    cnt = np.array([3, 0, 5, 1], np.int32)                          # ragged, one game without a record
    states = rng.integers(0, 2 ** 63, (4, 6, 2)).astype(np.uint64)
    pis, vs = rng.random((4, 6, 7), np.float32), rng.random((4, 6), np.float32)
    off, fs, fp, fv = fg.flatten_eval_log(cnt, states, pis, vs)
    assert off.tolist() == [0, 3, 3, 8, 9]
    for flat, logged in ((fs, states), (fp, pis), (fv, vs)):
        assert flat.dtype == logged.dtype and flat.flags["C_CONTIGUOUS"]
        assert np.array_equal(flat, np.array([logged[g, i] for g in range(4) for i in range(cnt[g])], logged.dtype).reshape(flat.shape))


class _Session:
    """selfplay_begin / selfplay_next / selfplay_full_plies / selfplay_end of an engine that replays slices of `one`"""

    def __init__(self, one):
        self.one, self.lo, self.off, self.open, self.begun = one, 0, 0, False, None

    def selfplay_begin(self, **kw):
        self.begun, self.open = kw, True

    def selfplay_next(self, k):
        assert self.open
        one, lo = self.one, self.lo
        cnt = 2 * tw.popcount(one["full_masks"][lo:lo + k])
        out = {key: one[key][self.off:self.off + cnt].copy() for key in ("boards", "pis", "zs")}
        out.update(count=cnt, game_len=one["game_len"][lo:lo + k].copy(), moves=one["moves"][lo:lo + k].copy())
        self.masks = one["full_masks"][lo:lo + k].copy()
        self.lo, self.off = lo + k, self.off + cnt
        return out

    def selfplay_full_plies(self):
        return self.masks

    def selfplay_end(self):
        self.open = False


CHUNKS = ((0, 2), (2, 3), (5, 1))


def test_session_in_chunks_passes_on_slices_of_the_one_call_run(ref):
    s = _Session(ref)
    fg.check_session_in_chunks(s, ref, CHUNKS, dict(n_games=6, seed=11))
    assert s.begun == dict(n_games=6, seed=11) and not s.open and s.lo == 6


@pytest.mark.parametrize("field", ["moves", "full_masks", "pis", "game_len"])
def test_session_in_chunks_fails_on_one_altered_chunk(ref, field):
    class Altered(_Session):
        def selfplay_next(self, k):
            out = super().selfplay_next(k)
            if self.lo == 5:                                        # the second chunk
                if field == "full_masks":
                    self.masks[0] ^= np.uint64(1 << 40)             # a ply no game reaches: the count stays
                elif field == "pis":
                    _one_ulp(out)
                else:
                    _bump(out[field], 1 if field == "game_len" else (1, 0))
            return out
    s = Altered(ref)
    with pytest.raises(AssertionError):
        fg.check_session_in_chunks(s, ref, CHUNKS, {})
    assert not s.open                                               # the session is closed behind a failure too
