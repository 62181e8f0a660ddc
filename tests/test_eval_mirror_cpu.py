"""The opt-in "eval_mirror" without a GPU: csrc/az_mirror.h (its g++ build) against the oracle's mirror and the plain-Python twin
(tests/mirror_twin.py), and the property the feature rests on -- a search over the mirror-canonical function F is an ordinary search
over an ordinary net, so its recorded rows replay on the unchanged oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alphazero-rs_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mirror_twin as mt      # noqa: E402


def _bit(c, r):
    return 1 << (c * 7 + r)


def _stack(cols):
    """cols[c] = string of 'x' (mine) / 'o' (theirs) from the bottom up"""
    mine = theirs = 0
    for c, col in enumerate(cols):
        for r, ch in enumerate(col):
            if ch == "x":
                mine |= _bit(c, r)
            else:
                theirs |= _bit(c, r)
    return mine, theirs


SYMMETRIC = [_stack(["", "", "", "x", "", "", ""]), _stack(["o", "", "", "x", "", "", "o"]), _stack(["x", "o", "", "", "", "o", "x"]),
             _stack(["", "", "xo", "ox", "xo", "", ""]), _stack(["xoxoxo", "", "", "", "", "", "xoxoxo"]),
             _stack(["x", "o", "x", "oxo", "x", "o", "x"]), _stack(["", "ox", "", "xoxoxo", "", "ox", ""]),
             _stack(["xo", "xo", "ox", "", "ox", "xo", "xo"])]
FULL = _stack(["xoxoxo", "oxoxox", "xoxoxo", "xoxoxo", "oxoxox", "xoxoxo", "oxoxox"])


@pytest.fixture(scope="module")
def positions(oracle):
    """>= 20,000 legal positions of all plies (random play-outs with the oracle's c4_play, terminal positions included), then the
    empty board, the hand-made self-symmetric positions and a full board."""
    rng = np.random.default_rng(11)
    out = []
    while len(out) < 20000:
        s = (0, 0)
        for _ in range(42):
            vm = oracle.c4_valid_mask(*s)
            s = oracle.c4_play(s[0], s[1], int(rng.choice([a for a in range(7) if (vm >> a) & 1])))
            out.append(s)
            if oracle.c4_ended(*s) != 0.0:
                break
    out += [(0, 0)] + SYMMETRIC + [FULL]
    return np.array(out, np.uint64)


@pytest.fixture(scope="module")
def header(tmp_path_factory, positions):
    """csrc/az_mirror.h through g++ on `positions`: [n, 8] words (tests/cpp/test_mirror_cpu.cpp)"""
    d = tmp_path_factory.mktemp("mirror")
    exe = str(d / "test_mirror_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_mirror_cpu.cpp"), "-o", exe])
    positions.tofile(str(d / "in.bin"))
    subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
    out = np.fromfile(str(d / "out.bin"), np.uint64).reshape(-1, 8)
    assert out.shape[0] == positions.shape[0]
    return out


def test_positions_cover_all_plies_and_the_special_cases(positions):
    stones = np.array([bin(int(m) | int(t)).count("1") for m, t in positions])
    assert set(range(0, 43)) - set(stones.tolist()) == set(), sorted(set(range(43)) - set(stones.tolist()))
    for s in SYMMETRIC + [(0, 0)]:
        assert mt.mirror(s) == s
    assert FULL[0] | FULL[1] == sum(0x3F << (7 * c) for c in range(7)) and mt.mirror(FULL) != FULL


def test_mirror_equals_the_oracle_and_is_an_involution(oracle, positions, header):
    L = oracle.lib()
    for (m, t), h in zip(positions, header):
        assert int(h[0]) == L.azo_c4_mirror(int(m)) and int(h[1]) == L.azo_c4_mirror(int(t))
        assert L.azo_c4_mirror(int(h[0])) == int(m) and L.azo_c4_mirror(int(h[1])) == int(t)
        assert mt.mirror_bits(int(h[0])) == int(m) and mt.mirror_bits(int(h[1])) == int(t)


def test_canonical_agrees_with_the_twin(positions, header):
    c, flags = mt.canonical_batch(positions)
    for i in range(0, len(positions), 7):                         # the twin's array form is its scalar form
        cs, f = mt.canonical(positions[i])
        assert cs == (int(c[i, 0]), int(c[i, 1])) and f == int(flags[i])
    assert np.array_equal(header[:, 4:6], c) and np.array_equal(header[:, 6], flags.astype(np.uint64))
    keys = np.array([mt.pack(m, t) for m, t in positions], np.uint64)
    mkeys = np.array([mt.pack(*mt.mirror(s)) for s in positions], np.uint64)
    assert np.array_equal(header[:, 2], keys)
    assert np.array_equal(header[:, 3], mkeys)                    # the pack word mirrors like a bitboard
    assert np.array_equal(header[:, 7], flags.astype(np.uint64))  # "mirrored" from the key alone, as the backup recomputes it
    assert 0.3 < flags.mean() < 0.7                               # both orientations occur


def test_canonical_of_the_mirror_is_the_same_state_with_the_opposite_flag(positions, header, tmp_path):
    mirrored = mt.mirror_batch(positions)
    c2, f2 = mt.canonical_batch(mirrored)
    assert np.array_equal(c2, header[:, 4:6])
    sym = np.all(mirrored == positions, axis=1)
    assert sym.sum() >= len(SYMMETRIC) + 1
    assert np.all(header[sym, 6] == 0) and np.all(f2[sym] == 0)
    assert np.array_equal(f2[~sym].astype(np.uint64), 1 - header[~sym, 6])
    # ... and by the header itself, on the mirrored inputs
    exe_dir = tmp_path
    exe = str(exe_dir / "t")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_mirror_cpu.cpp"), "-o", exe])
    mirrored.tofile(str(exe_dir / "in.bin"))
    subprocess.check_call([exe, str(exe_dir / "in.bin"), str(exe_dir / "out.bin")])
    h2 = np.fromfile(str(exe_dir / "out.bin"), np.uint64).reshape(-1, 8)
    assert np.array_equal(h2[:, 4:6], header[:, 4:6])
    assert np.all(h2[sym, 6] == 0) and np.array_equal(h2[~sym, 6], 1 - header[~sym, 6])


def test_valid_mask_of_the_mirror_is_the_bit_reversed_mask(oracle, positions, header):
    for (m, t), h in zip(positions, header):
        vm = oracle.c4_valid_mask(int(m), int(t))
        rev = sum(((vm >> a) & 1) << (6 - a) for a in range(7))
        assert oracle.c4_valid_mask(int(h[0]), int(h[1])) == rev


# ---- the property the feature rests on, on the oracle alone ---------------------------------------------------------------------------
class AsymmetricNet:
    """A fixed random linear-softmax net on the 84 features: nothing in it is mirror-symmetric."""

    def __init__(self, seed=3):
        rng = np.random.default_rng(seed)
        self.w = rng.standard_normal((84, 7)).astype(np.float32)
        self.wv = rng.standard_normal(84).astype(np.float32) * np.float32(0.3)

    def __call__(self, states):
        x = mt.states_to_boards(states).reshape(-1, 84)
        z = (x @ self.w).astype(np.float32)
        e = np.exp(z - z.max(axis=1, keepdims=True)).astype(np.float32)
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), np.tanh(x @ self.wv).astype(np.float32)


def test_twin_f_is_equivariant_and_the_net_is_not(positions):
    net = AsymmetricNet()
    s = positions[::40]
    pi, v = mt.f_from_n(net, s)
    pim, vm = mt.f_from_n(net, mt.mirror_batch(s))
    # a self-symmetric position IS its own mirror image (c(s) = s, not mirrored): there F(mirror(s)) is F(s) itself, not its reverse
    sym = np.all(mt.mirror_batch(s) == s, axis=1)
    assert sym.any() and not sym.all()
    assert np.array_equal(pim[~sym], pi[~sym][:, ::-1]) and np.array_equal(pim[sym], pi[sym])
    assert np.array_equal(vm.view(np.uint32), v.view(np.uint32))
    rp, rv = net(s[~sym])
    rpm, rvm = net(mt.mirror_batch(s[~sym]))
    assert not np.array_equal(rpm, rp[:, ::-1]) and not np.array_equal(rvm, rv)


def test_a_search_over_f_replays_on_the_unchanged_oracle(oracle):
    """64 games x 25 sims with NET_CALLBACK and the twin's F over the asymmetric net; the requested rows, fed back with NET_REPLAY, give
    the same games."""
    n, sims, seed = 64, 25, 5
    net = AsymmetricNet()
    rows = {"s": [], "pi": [], "v": []}

    def predict(boards, model_id):
        st = mt.boards_to_states(boards)
        pi, v = mt.f_from_n(net, st)
        rows["s"].append(st.copy()); rows["pi"].append(pi.copy()); rows["v"].append(v.copy())
        return pi, v

    oracle.set_predict_callback(predict)
    games, off = [], [0]
    for g in range(n):                        # one episode per call: the rows of a call are the episode's, in order
        games.append(oracle.selfplay(1, sims, net_kind=oracle.NET_CALLBACK, seed=seed, first_game_id=g, threads=1))
        off.append(sum(len(x) for x in rows["v"]))
    fs, fp, fv = np.concatenate(rows["s"]), np.concatenate(rows["pi"]), np.concatenate(rows["v"])
    ref = oracle.selfplay(n, sims, net_kind=oracle.NET_REPLAY, seed=seed, threads=4, replay=(np.array(off, np.int64), fs, fp, fv))
    assert not ref["replay_bad"].any()
    assert np.array_equal(ref["game_len"], np.concatenate([g["game_len"] for g in games]))
    assert np.array_equal(ref["moves"], np.concatenate([g["moves"] for g in games]))
    assert np.array_equal(ref["pis"], np.concatenate([g["pis"] for g in games]))
    assert np.array_equal(ref["zs"], np.concatenate([g["zs"] for g in games]))
    # the trees asked for both orientations; F answered them from one
    distinct = {tuple(int(x) for x in s) for s in fs}
    canon = {mt.canonical(s)[0] for s in distinct}
    assert len(canon) < len(distinct)
