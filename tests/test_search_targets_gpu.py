"""Search statistics as training targets on the GPU ("selfplay_record_search", az_selfplay_get_search, az_samples_blend_z,
az_samples_surprise; include/az_engine.h): the record against the self-play twin (tests/selfplay_twin.py) and the
g++ build of csrc/az_target.h (tests/target_twin.py) bit for bit on every path that records, bit for bit WITHOUT effect where it must have
none, the two consumers against the g++ build, and the two Coaches.

Shapes follow the other feature modules: 100 episodes on 40 slots (one whole 256-lane tree workgroup plus one partial wave, with slot
refill), 25 simulations, the hash net as model 10.  The consumers run at the sizes of tests/test_search_targets_cpu.py: one tuple, the
workgroup edge and the 2048-wide scan block edge of az_draw.h."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch                   # before the engine library is loaded: torch brings its own HIP runtime, and a process wants one

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg        # noqa: E402
import selfplay_twin as tw      # noqa: E402
import target_twin as tt        # noqa: E402
from feature_gpu import AZ_ERR_BAD_ARGUMENT, COUNTERS, HASH_SALT, N_GAMES, oracle_salt      # noqa: E402

SIMS, SEED, FIRST = 25, 5, 1000
CONFIGS = {"plain": dict(), "noise": dict(noise=(0.25, 1.0)), "forced": dict(forced=(2.0, True))}
COPY_SIZES = (1, 2, 257, 2047, 2048, 2049, 5000)
FULL_TOP = sum(1 << (c * 7 + 5) for c in range(7))


@pytest.fixture(autouse=True)
def options_off_afterwards(engine):
    """The session's engine is shared with every other module: leave it as it was found."""
    yield
    fg.restore(engine)
    engine.set_gumbel(0)
    engine.set_option("selfplay_record_search", 0)


def recorded(e, sims=SIMS, seed=SEED, **kw):
    """One run_selfplay with the option on, plus its search rows."""
    if kw.get("threads", 1) > 1:
        sims = 24                                                              # num_sims % num_sim_threads == 0
    e.set_option("selfplay_record_search", 1)
    got = fg.run_selfplay(e, sims, seed, first_game_id=FIRST, **kw)
    got["root_q"], got["root_prior"] = e.selfplay_search()
    return got


def same_bits(a, b):
    return fg.same_rows(np.ascontiguousarray(a), np.ascontiguousarray(b))


def twin_rows(got, noise=None, forced=None):
    """One tw.Tree per episode walks the recorded moves: (pi, root_prior, R) per ply, in the order of the tuples without symmetries."""
    eps, alpha = noise or (0.0, 1.0)
    k, prune = forced or (0.0, False)
    pis, priors, rs = [], [], []
    for i, (ln, mv) in enumerate(zip(got["game_len"], got["moves"])):
        t = tw.Tree(SIMS, net_kind=tw.NET_HASH, salt=oracle_salt(10))
        mine, theirs = 0, 0
        for ply in range(int(ln)):
            pi, counts, q = t.get_action_prob(mine, theirs, 1.0 if ply + 1 < 15 else 0.0, seed=SEED, game_id=FIRST + i, eps=eps, alpha=alpha, k=k,
                                              prune=int(prune))
            pis.append(pi)
            priors.append(t.root_priors(mine, theirs))
            rs.append(tt.root_value_py(counts, q))
            mine, theirs = fg.c4_play(mine, theirs, int(mv[ply]))
        t.close()
    return np.array(pis, np.float32), np.array(priors, np.float32), np.array(rs, np.float32)


_reference = {}


def reference(engine, name):
    """The one-call run of a configuration with symmetries (computed once, shared, left unchanged) and the twin's rows for it."""
    if name not in _reference:
        got = recorded(engine, **CONFIGS[name])
        fg.restore(engine)
        _reference[name] = (got, twin_rows(got, CONFIGS[name].get("noise"), CONFIGS[name].get("forced")))
    return _reference[name]


# ---- the record against the twin ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_record_equals_the_twin(engine, name):
    got, (pis, priors, rs) = reference(engine, name)
    n = int(got["game_len"].sum())
    assert got["count"] == 2 * n == len(got["root_q"]) == len(got["root_prior"]) and len(rs) == n
    assert same_bits(got["pis"][0::2], pis)                                    # at every ply the twin's pi is the engine's
    assert same_bits(got["root_prior"][0::2], priors)
    assert same_bits(got["root_q"][0::2], rs)
    assert same_bits(got["root_prior"][1::2], priors[:, ::-1])                 # the mirrored tuple: its prior reversed, its R the same
    assert same_bits(got["root_q"][1::2], rs)
    assert np.all(np.abs(got["root_q"]) <= 1.0) and np.any(got["root_q"] != 0.0)
    if name == "noise":                                                        # the prior as the search used it: noise included
        plain = reference(engine, "plain")[1][1]
        assert not np.array_equal(priors[0], plain[0])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_record_without_symmetries_and_in_chunks(engine, name):
    one, _ = reference(engine, name)
    got = recorded(engine, symmetries=False, **CONFIGS[name])
    assert got["count"] * 2 == one["count"]
    assert same_bits(got["pis"], one["pis"][0::2]) and same_bits(got["root_q"], one["root_q"][0::2])
    assert same_bits(got["root_prior"], one["root_prior"][0::2])
    check_chunks(engine, one, dict(num_sims=SIMS, model_id=10, seed=SEED, first_game_id=FIRST, concurrent=fg.SLOTS))


def check_chunks(engine, one, begin_kwargs, chunks=((0, 30), (30, 30), (60, 40))):
    """A session fetched in chunks returns the slices of the one-call run `one` -- tuples and search rows (option still on)."""
    per_game = 2 * one["game_len"].astype(np.int64)
    engine.selfplay_begin(N_GAMES, **begin_kwargs)
    try:
        off = 0
        for lo, k in chunks:
            got = engine.selfplay_next(k)
            q, prior = engine.selfplay_search()
            cnt = int(per_game[lo:lo + k].sum())
            assert got["count"] == cnt == len(q) == len(prior)
            for key in ("states", "pis", "zs"):
                assert same_bits(got[key], one[key][off:off + cnt]), key
            assert same_bits(q, one["root_q"][off:off + cnt]) and same_bits(prior, one["root_prior"][off:off + cnt])
            off += cnt
        assert off == one["count"]
    finally:
        engine.selfplay_end()


@pytest.mark.parametrize("variant", [dict(options={"fused_search": 0}), dict(options={"fused_search": 1}), dict(threads=2),
                                     dict(options={"eval_dedup": 2, "fused_search": 0})])
def test_paths_record_the_same_rows_as_their_own_one_call_run(engine, variant):
    one = recorded(engine, **variant)
    assert one["count"] == len(one["root_q"]) > 0
    if variant.get("threads", 1) == 1:                                         # one simulation in flight: the plain reference's rows
        ref, _ = reference(engine, "plain")
        engine.set_option("selfplay_record_search", 1)
        for k, v in variant.get("options", {}).items():
            engine.set_option(k, v)
        assert same_bits(one["pis"], ref["pis"]) and same_bits(one["root_q"], ref["root_q"]) and same_bits(one["root_prior"], ref["root_prior"])
    check_chunks(engine, one, dict(num_sims=24 if variant.get("threads", 1) > 1 else SIMS, model_id=10, seed=SEED, first_game_id=FIRST,
                                   concurrent=fg.SLOTS, num_sim_threads=variant.get("threads", 1)))


def test_connect_three_records(engine_mod):
    """The seam's second game: rows for every tuple, priors zero on full columns and summing to 1, |R| <= 1."""
    for e in fg.connect_three_engine(engine_mod):
        got = recorded(e)
        check_consistency(got)


# ---- off means off; on changes no tuple ---------------------------------------------------------------------------------------------------
def test_off_equals_never_set_and_on_changes_no_tuple(engine_mod):
    runs = []
    for touch in (None, 0, 1):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
        try:
            e.net_set_kind(10, engine_mod.NET_HASH, HASH_SALT)
            e.net_set_kind(11, engine_mod.NET_HASH, HASH_SALT)
            if touch is not None:
                e.set_option("selfplay_record_search", 1)
                e.set_option("selfplay_record_search", touch)
            got = fg.run_selfplay(e, SIMS, SEED, first_game_id=FIRST, cap=(10, 250000))
            if touch == 1:
                q, prior = e.selfplay_search()
                assert len(q) == got["count"]
            else:
                with pytest.raises(engine_mod.AzError) as ei:
                    e.selfplay_search()
                assert ei.value.status == AZ_ERR_BAD_ARGUMENT
            e.reset_stats()
            other = fg.other_entry_points(e)
            runs.append((got, other, e.stats()))
        finally:
            e.close()
    base = runs[0]
    for got, other, st in runs[1:]:
        for key in ("count", "game_len", "moves", "states", "boards", "pis", "zs", "full_masks"):
            assert np.array_equal(got[key], base[0][key]), key
        for key in COUNTERS:
            assert got["stats"][key] == base[0]["stats"][key], key
            assert st[key] == base[2][key], key
        fg.assert_same_outputs(other, base[1])


def test_option_range_open_session_and_async(engine, engine_mod):
    fg.check_option_ranges(engine, engine_mod, bad=(("selfplay_record_search", (-1, 2, 1000000)),), good=(("selfplay_record_search", (0, 1)),),
                           settle=lambda: engine.set_option("selfplay_record_search", 0),
                           locked=(("selfplay_record_search", 1), ("selfplay_record_search", 0)), reopen=("selfplay_record_search", 1))
    engine.set_option("selfplay_async", 1)
    for call in (lambda: engine.selfplay(n_games=8, num_sims=10, model_id=10, seed=1), lambda: engine.selfplay_begin(8, 10, 10, seed=1)):
        with pytest.raises(engine_mod.AzError) as ei:
            call()
        assert ei.value.status == AZ_ERR_BAD_ARGUMENT
    engine.set_option("selfplay_record_search", 0)
    engine.selfplay(n_games=8, num_sims=10, model_id=10, seed=1)               # the free-running path itself is untouched
    with pytest.raises(engine_mod.AzError):
        engine.selfplay_search()                                               # ... and that call ran with the option off


# ---- no twin records there: consistency ---------------------------------------------------------------------------------------------------
def check_consistency(got):
    q, prior = got["root_q"], got["root_prior"]
    assert len(q) == len(prior) == got["count"] > 0
    assert np.all(np.abs(q) <= 1.0)
    assert np.all(prior >= 0.0)
    s = np.asarray(got["states"], np.uint64)
    top = (s[:, 0] | s[:, 1]) & np.uint64(FULL_TOP)
    full = np.array([[(int(t) >> (c * 7 + 5)) & 1 for c in range(7)] for t in top], bool)
    assert np.all(prior[full] == 0.0)
    assert np.all(np.abs(prior.astype(np.float64).sum(axis=1) - 1.0) <= 1e-5)


def test_playout_cap_and_gumbel_rows_are_consistent(engine):
    got = recorded(engine, sims=50, cap=(20, 250000))
    assert got["count"] == 2 * tw.popcount(got["full_masks"]) < 2 * int(got["game_len"].sum())
    check_consistency(got)
    fg.restore(engine)
    engine.set_gumbel(4)
    got = recorded(engine, sims=16)
    check_consistency(got)


# ---- the consumers against the g++ build ----------------------------------------------------------------------------------------------------
def consumer_inputs(n):
    """The CPU test's pis and priors, plus legal positions (random playouts from the initial board), zs and root values."""
    pis, priors = tt.copy_inputs(n)
    rng = np.random.default_rng(11)
    states = np.zeros((n, 2), np.uint64)
    for i in range(n):
        mine, theirs = 0, 0
        for _ in range(int(rng.integers(0, 12))):
            cols = [c for c in range(7) if not ((mine | theirs) >> (c * 7 + 5)) & 1]
            mine, theirs = fg.c4_play(mine, theirs, int(rng.choice(cols)))
        states[i] = (mine, theirs)
    zs = rng.choice(np.array([-1.0, 1.0, 1e-4, -1e-4], np.float32), n)
    rq = rng.uniform(-1, 1, n).astype(np.float32)
    return pis, priors, states, zs, rq


@pytest.mark.parametrize("n", COPY_SIZES)
def test_blend_z_equals_the_twin(engine, n):
    _, _, _, zs, rq = consumer_inputs(n)
    for lam in (0.0, 0.5, 0.25, 1.0):
        want = tt.blend(zs, rq, lam)
        assert same_bits(engine.blend_z(zs, rq, lam), want), lam
        dz, dr = torch.from_numpy(zs).cuda(), torch.from_numpy(rq).cuda()
        out = torch.full((n,), 7.0, device="cuda")
        engine.blend_z(dz, dr, lam, out=out)
        assert same_bits(out.cpu().numpy(), want), lam
        engine.blend_z(dz, dr, lam, out=dz)                                    # zs_out == zs, on the device
        assert same_bits(dz.cpu().numpy(), want), lam
        hz = zs.copy()
        engine.blend_z(hz, rq, lam, out=hz)                                    # ... and on the host
        assert same_bits(hz, want), lam
    assert len(engine.blend_z(np.zeros(0, np.float32), np.zeros(0, np.float32), 0.5)) == 0      # n = 0 is legal


def test_blend_z_refusals_write_nothing(engine, engine_mod):
    zs, rq = np.array([1.0, -1.0, 0.5], np.float32), np.array([0.1, 0.2, 0.3], np.float32)
    bad_inputs = [(zs, rq, 1.000001), (zs, rq, -0.000001), (np.array([1.0, np.nan, 0.5], np.float32), rq, 0.5),
                  (zs, np.array([0.1, np.nan, 0.3], np.float32), 0.5), (np.array([1.0, 1.5, 0.5], np.float32), rq, 0.5),
                  (zs, np.array([0.1, -1.01, 0.3], np.float32), 0.5)]
    for z, r, lam in bad_inputs:
        out = np.full(3, 7.0, np.float32)
        with pytest.raises(engine_mod.AzError) as ei:
            engine.blend_z(z, r, lam, out=out)
        assert ei.value.status == AZ_ERR_BAD_ARGUMENT and np.all(out == 7.0)
    out = np.full(3, 7.0, np.float32)
    assert engine._lib.az_samples_blend_z(engine._h, -1, engine_mod._ptr(zs), engine_mod._ptr(rq), 500000, engine_mod._ptr(out)) == AZ_ERR_BAD_ARGUMENT
    engine.selfplay_begin(4, 10, 10, seed=1)
    try:
        with pytest.raises(engine_mod.AzError) as ei:
            engine.blend_z(zs, rq, 0.5, out=out)
        assert ei.value.status == AZ_ERR_BAD_ARGUMENT
    finally:
        engine.selfplay_end()
    assert np.all(out == 7.0)


@pytest.mark.parametrize("share", [0.5, 1.0])
@pytest.mark.parametrize("n", COPY_SIZES)
def test_surprise_equals_the_twin(engine, n, share):
    from alphazero_rs_amd.coach import states_to_boards
    pis, priors, states, zs, _ = consumer_inputs(n)
    boards = states_to_boards(states)
    want = tt.surprise(pis, priors, share, 1)
    e_states, e_boards, e_pis, e_zs = tt.expand(want["counts"], states, boards, pis, zs)
    stats0 = engine.stats()
    routes = {"states": dict(states=states), "boards": dict(boards=boards), "both": dict(states=states, boards=boards),
              "device": dict(states=torch.from_numpy(states.view(np.int64)).cuda())}
    for route, kw in routes.items():
        dev = route == "device"
        args = [torch.from_numpy(a).cuda() for a in (pis, zs, priors)] if dev else [pis, zs, priors]
        got = engine.surprise(args[0], args[1], args[2], share, 1, **kw)
        assert np.array_equal(got["counts"], want["counts"]), route
        assert same_bits(got["kl"], want["kl"]), route
        assert got["count"] == want["total"] == len(got["zs"]), route
        assert same_bits(got["pis"], e_pis) and same_bits(got["zs"], e_zs), route
        if "states" in kw:
            assert same_bits(got["states"], e_states), route
        if "boards" in kw:
            assert same_bits(got["boards"], e_boards), route
    only = engine.surprise(pis, zs, priors, share, 1, states=states, want=False)   # dst = NULL: the counts and KL alone
    assert np.array_equal(only["counts"], want["counts"]) and "pis" not in only
    same = engine.surprise(pis, zs, pis, 1.0, 1, states=states)                     # pi == prior everywhere: the input unchanged
    zero = engine.surprise(pis, zs, priors, 0.0, 1, states=states)                  # share = 0: the same
    for r in (same, zero):
        assert np.all(r["counts"] == 1) and same_bits(r["pis"], pis) and same_bits(r["zs"], zs) and same_bits(r["states"], states)
    stats1 = engine.stats()
    for key in COUNTERS:                                                       # pure: every counter but device_ms stays
        assert stats0[key] == stats1[key], key


def test_surprise_refusals_write_nothing(engine, engine_mod):
    from alphazero_rs_amd.coach import states_to_boards
    n = 300
    pis, priors, states, zs, _ = consumer_inputs(n)
    boards = states_to_boards(states)
    lib, h, az_samples, ptr = engine._lib, engine._h, engine_mod.az_samples, engine_mod._ptr
    out = {"states": np.full((2 * n, 2), 9, np.uint64), "pis": np.full((2 * n, 7), 7.0, np.float32), "zs": np.full(2 * n, 7.0, np.float32),
           "counts": np.full(n, 9, np.uint32), "kl": np.full(n, 7.0, np.float32)}

    def call(pis=pis, zs=zs, priors=priors, states=states, boards=None, share_e6=500000, count=n, cap=2 * n, dst_pis=None):
        src = az_samples(count, count, ptr(states), ptr(boards), ptr(pis), ptr(zs), None, None)
        dst = az_samples(cap, 0, ptr(out["states"]) if states is not None else None, None, ptr(out["pis"] if dst_pis is None else dst_pis),
                         ptr(out["zs"]), None, None)
        return lib.az_samples_surprise(h, C.byref(src), ptr(priors), share_e6, 1, C.byref(dst), ptr(out["counts"]), ptr(out["kl"]))

    def spoil(a, idx, v):
        b = a.copy()
        b[idx] = v
        return b
    overlap = np.zeros((2 * n, 7), np.float32)
    overlap[:n] = pis
    bad_board = spoil(boards, (5, 0, 2, 3), 0.5)
    stones_twice, off_board = states.copy(), states.copy()
    stones_twice[9] = (1, 1)
    off_board[9] = (1 << 6, 0)
    both_planes = boards.copy()
    both_planes[7, 0, 5, 0] = both_planes[7, 1, 5, 0] = 1.0
    cases = {"nan pi": dict(pis=spoil(pis, (3, 2), np.nan)), "pi > 1": dict(pis=spoil(pis, (3, 2), 1.5)), "z": dict(zs=spoil(zs, 299, -1.5)),
             "nan z": dict(zs=spoil(zs, 0, np.nan)), "prior < 0": dict(priors=spoil(priors, (257, 6), -0.1)),
             "prior > 1": dict(priors=spoil(priors, (0, 0), 1.5)), "nan prior": dict(priors=spoil(priors, (0, 0), np.nan)),
             "overlapping stones": dict(states=stones_twice), "off-board bit": dict(states=off_board),
             "feature": dict(states=None, boards=bad_board), "both planes": dict(states=None, boards=both_planes),
             "share < 0": dict(share_e6=-1), "share > 1": dict(share_e6=1000001), "capacity": dict(cap=2 * n - 1), "n < 0": dict(count=-1),
             "n > 2^24": dict(count=(1 << 24) + 1, cap=(1 << 26)), "overlap": dict(pis=overlap[:n], dst_pis=overlap)}
    for name, kw in cases.items():
        assert call(**kw) == AZ_ERR_BAD_ARGUMENT, name
    engine.selfplay_begin(4, 10, 10, seed=1)
    try:
        assert call() == AZ_ERR_BAD_ARGUMENT
    finally:
        engine.selfplay_end()
    assert np.all(out["states"] == 9) and np.all(out["pis"] == 7.0) and np.all(out["zs"] == 7.0) and np.all(out["counts"] == 9) and np.all(out["kl"] == 7.0)
    assert np.array_equal(overlap[:n], pis) and np.all(overlap[n:] == 0.0)
    assert call() == 0                                                           # and the same call with nothing wrong goes through


def test_consumers_are_refused_while_a_training_session_is_open(engine_mod):
    pis, priors, states, zs, rq = consumer_inputs(64)
    e = engine_mod.Engine(device=0, max_batch=64, net_channels=128)
    try:
        e.net_init_random(0, 3)
        e.train_begin(0)
        for call in (lambda: e.blend_z(zs, rq, 0.5), lambda: e.surprise(pis, zs, priors, 0.5, 1, states=states)):
            with pytest.raises(engine_mod.AzError) as ei:
                call()
            assert ei.value.status == AZ_ERR_BAD_ARGUMENT
        e.train_end(1)
        assert same_bits(e.blend_z(zs, rq, 0.5), tt.blend(zs, rq, 0.5))
    finally:
        e.close()


# ---- the two Coaches ------------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_coach_agree_with_targets(engine_mod, tmp_path):
    """One iteration, C = 128, 32 episodes, value_target_q = 0.5 and surprise_share = 0.5 on both hosts: same report, byte-identical files,
    and a 0.examples that differs from the plain run's; the option is on for the episodes only."""
    from alphazero_rs_amd.coach import Coach, load_examples
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp", "plain")}
    seen = []

    def run_py(d, on):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
        try:
            e.net_init_random(0, 3)
            e.set_option("train_epochs", 1)
            coach = Coach.setup(e, d, 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 1, 32, 25, 1, 1000, 1, log=lambda m: None)
            if on:
                coach.value_target_q, coach.surprise_share = 0.5, 0.5
                orig_set, orig_arena = e.set_option, e.arena

                def spy(key, value):
                    if key == "selfplay_record_search":
                        seen.append((key, value))
                    return orig_set(key, value)

                def arena_spy(*a, **kw):
                    seen.append(("arena", 0))
                    return orig_arena(*a, **kw)
                e.set_option, e.arena = spy, arena_spy
            return coach.learn(seed=11)
        finally:
            e.close()
    rep = run_py(dirs["py"], True)
    run_py(dirs["plain"], False)
    exe = os.path.join(tmp_path, "test_coach_targets")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_targets.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, dirs["cpp"], "128", "11", "value_target_q=0.5", "surprise_share=0.5"], check=True, stdout=subprocess.PIPE, text=True,
                         timeout=600).stdout
    crep = json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    assert len(rep) == len(crep) == 1
    for k in fg.REPORT_KEYS:
        assert rep[0][k] == crep[0][k], k
    fg.compare_directories(dirs["py"], dirs["cpp"])
    with open(os.path.join(dirs["py"], "0.examples"), "rb") as x, open(os.path.join(dirs["plain"], "0.examples"), "rb") as y:
        assert x.read() != y.read()
    assert seen == [("selfplay_record_search", 1), ("selfplay_record_search", 0), ("arena", 0)], seen
    (_, _, vs), = load_examples(os.path.join(dirs["py"], "0.examples"))
    assert np.all(np.abs(vs) <= 1.0) and np.any((np.abs(vs) != 1.0) & (np.abs(vs) != np.float32(1e-4)))      # blended zs are on disk
