"""Playout cap randomization without a GPU ("playout_cap_sims" / "playout_cap_full_e6", include/az_engine.h): the predicate of
csrc/az_playout.h in its g++ build against a Python restatement, the twin (tests/cpp/selfplay_twin.cpp) against the unchanged oracle
where the two must agree, the twin's own bookkeeping, and the new export and keys in every place that names the ABI."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import selfplay_twin as pc      # noqa: E402

HASH_SALT = 1234
KEYS = ("playout_cap_sims", "playout_cap_full_e6")
EXPORT = "az_selfplay_get_full_plies"


# ---- 1. the predicate --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_e6", [0, 1, 250000, 500000, 999999, 1000000])
def test_host_predicate_equals_the_python_restatement(full_e6):
    assert pc.lib().twin_playout_thresh24(full_e6) == (full_e6 << 24) // 1000000
    for seed in (11, 12):
        gids, plies = np.meshgrid(np.arange(48, dtype=np.uint64), np.arange(42, dtype=np.uint64), indexing="ij")
        # episode ids as a Coach numbers them (iteration x num_eps + index) are covered by a second, far-away block
        for first in (0, 1000, 2 ** 40 + 7):
            g = gids.reshape(-1) + np.uint64(first)
            got = pc.full_host(seed, g, plies.reshape(-1), full_e6)
            want = np.array([pc.full_py(seed, int(a), int(b), full_e6) for a, b in zip(g, plies.reshape(-1))])
            assert np.array_equal(got, want), (seed, first, full_e6)
            if full_e6 == 0:
                assert not got.any()
            if full_e6 == 1000000:
                assert got.all()


def test_predicate_shares_of_the_issue_table():
    """The seeds and P the GPU tests use are far from degenerate: the share of full moves over 48 episodes x 42 plies, and the number of
    episodes that start with a full move."""
    for seed, full_e6, starts in ((11, 250000, 14), (11, 500000, 23), (12, 250000, 13), (12, 500000, 24)):
        gids, plies = np.meshgrid(np.arange(48, dtype=np.uint64), np.arange(42, dtype=np.uint64), indexing="ij")
        m = pc.full_host(seed, gids.reshape(-1), plies.reshape(-1), full_e6).reshape(48, 42)
        assert abs(m.mean() - full_e6 / 1e6) < 0.03, (seed, full_e6, m.mean())
        assert int(m[:, 0].sum()) == starts, (seed, full_e6, int(m[:, 0].sum()))


# ---- 2. every move full: the twin is the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("net", ["stub", "hash"])
def test_twin_with_every_move_full_equals_the_oracle(oracle, net, threads):
    kind, okind, salt = (pc.NET_STUB, oracle.NET_STUB, 0) if net == "stub" else (pc.NET_HASH, oracle.NET_HASH, HASH_SALT)
    n, sims = 12, 24
    ref = oracle.selfplay(n, sims, net_kind=okind, salt=salt, seed=11, first_game_id=5, sim_threads=threads)
    got = pc.selfplay(n, sims, cap_sims=8, full_e6=1000000, net_kind=kind, salt=salt, seed=11, first_game_id=5, sim_threads=threads)
    assert got["count"] == ref["count"] == 2 * int(ref["game_len"].sum())
    assert np.array_equal(got["game_len"], ref["game_len"]) and np.array_equal(got["moves"], ref["moves"])
    assert np.array_equal(got["boards"], ref["boards"])
    assert np.array_equal(got["pis"].view(np.uint32), ref["pis"].view(np.uint32)) and np.array_equal(got["zs"], ref["zs"])
    assert [int(m) for m in got["full_masks"]] == [(1 << int(l)) - 1 for l in ref["game_len"]]
    assert got["sims"] == got["budgets"] == sims * int(ref["game_len"].sum())


# ---- 3. the twin's own bookkeeping -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sims,cap_sims,threads,game", [(24, 8, 1, "c4"), (24, 8, 4, "c4"), (44, 12, 1, "c4"), (25, 5, 1, "c3")])
def test_twin_at_a_quarter_full(oracle, sims, cap_sims, threads, game):
    n, seed, full_e6 = 48, 11, 250000
    kind = pc.GAME_CONNECT3 if game == "c3" else pc.GAME_BITS
    ended = oracle.c3_ended if game == "c3" else oracle.c4_ended
    r = pc.selfplay(n, sims, cap_sims=cap_sims, full_e6=full_e6, net_kind=pc.NET_HASH, salt=HASH_SALT, seed=seed, sim_threads=threads, game_kind=kind)
    full = pc.popcount(r["full_masks"])
    plies = int(r["game_len"].sum())
    assert r["count"] == 2 * full                                      # tuples = full plies x both symmetries
    for g in range(n):
        assert int(r["full_masks"][g]) >> int(r["game_len"][g]) == 0      # no full ply beyond the game's end
        for ply in range(int(r["game_len"][g])):
            assert bool((int(r["full_masks"][g]) >> ply) & 1) == pc.full_py(seed, g, ply, full_e6)
    assert r["sims"] == r["budgets"] == sims * full + cap_sims * (plies - full)
    # complete games under the oracle's rules: every move legal, the game over after the last move and not before
    for g in range(n):
        s = (0, 0)
        for ply in range(int(r["game_len"][g])):
            a = int(r["moves"][g, ply])
            assert (oracle.c4_valid_mask(*s) >> a) & 1, (g, ply)
            s = oracle.c4_play(s[0], s[1], a)
            assert (ended(*s) != 0.0) == (ply == int(r["game_len"][g]) - 1), (g, ply)
    # non-degenerate: both kinds of move, also at ply 0
    assert 0.1 <= full / plies <= 0.9
    first = [int(m) & 1 for m in r["full_masks"]]
    assert 0 < sum(first) < n
    # z of a recorded ply is the game's result from that ply's player: the two symmetries of a ply carry the same z
    assert np.array_equal(r["zs"][0::2], r["zs"][1::2])


def test_twin_with_no_full_move_emits_nothing():
    r = pc.selfplay(6, 24, cap_sims=8, full_e6=0, net_kind=pc.NET_HASH, salt=HASH_SALT, seed=12)
    assert r["count"] == 0 and not r["full_masks"].any() and (r["game_len"] >= 7).all()
    assert r["sims"] == r["budgets"] == 8 * int(r["game_len"].sum())


# ---- 4. the export and the keys, everywhere the ABI is written down -----------------------------------------------------------------------------
def test_export_and_keys_agree_everywhere(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"az_status\s+%s\s*\(([^)]*)\)\s*;" % EXPORT, code)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["az_engine* e", "uint64_t* mask"]
    rust = open(os.path.join(ROOT, "rust", "az-engine-sys", "src", "lib.rs")).read()
    sig = "pub fn %s(e: *mut az_engine, mask: *mut u64) -> c_int;" % EXPORT
    assert sig in rust
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert sig in "\n".join(re.findall(r"```rust\n(.*?)```", md, flags=re.S))
    assert EXPORT in engine_mod.EXPORTS
    lib = ctypes.CDLL(engine_mod.LIB_PATH)
    assert hasattr(lib, EXPORT)
    host = open(os.path.join(ROOT, "include", "az_host.hpp")).read()
    assert EXPORT in host and "set_playout_cap" in host and "selfplay_full_plies" in host
    assert hasattr(engine_mod.Engine, "set_playout_cap") and hasattr(engine_mod.Engine, "selfplay_full_plies")
    blob = open(engine_mod.LIB_PATH, "rb").read()
    pysrc = open(os.path.join(ROOT, "alphazero-rs_amd", "engine.py")).read()
    for key in KEYS:
        q = '"%s"' % key
        assert q in hdr and q in md and q in host and q in pysrc, key
        assert key.encode() + b"\0" in blob, key                        # the built library parses the key
    # the purpose word and the threshold formula are stated in the header as the shared text computes them
    assert "rng_draw(seed, game_id, ply, 6)" in hdr and "(P * 2^24) / 1000000" in hdr
    txt = open(os.path.join(ROOT, "alphazero-rs_amd", "csrc", "az_playout.h")).read()
    assert "RNG_PLAYOUT_CAP = 6" in txt


def test_both_coaches_carry_the_option():
    from alphazero_rs_amd import coach
    src = open(coach.__file__).read()
    host = open(os.path.join(ROOT, "include", "az_host.hpp")).read()
    for text in (src, host):
        assert "playout_cap_sims" in text and "playout_cap_full" in text
