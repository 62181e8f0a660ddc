"""Gumbel root search with sequential halving on the GPU ("gumbel_m" / "gumbel_c_visit_e6" / "gumbel_c_scale_e6", include/az_engine.h), held
to the project's bar: bit-exact against the twin (tests/cpp/gumbel_twin.cpp -- the unchanged oracle with the rule restated around it, and the
g++ build of csrc/az_gumbel.h, the text the kernels compile) on every path a Gumbel move can take, and bit for bit WITHOUT effect where it
must have none.

Shapes are the harness's small ones: 100 episodes on 40 slots = one whole 256-lane tree workgroup (32 games) plus one partial wave, with
slot refill; (m, simulations) = (2, 8), (4, 16), (7, 33); the stub net as model 0 and the hash net as model 10.  Every parity test asserts on
the twin's counters that the root selections it compared were not PUCT's, that moves were played whose selected action is not the most
visited one, that roots were reused with a non-zero baseline, and that both exploring (g != 0) and greedy (g = 0) moves were compared
(tests/test_gumbel_cpu.py asserts the same on the CPU alone for these seeds)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg        # noqa: E402
import gumbel_twin as gt        # noqa: E402
from feature_gpu import AZ_ERR_BAD_ARGUMENT, COUNTERS, HASH_SALT, N_GAMES, PER_SIM, SLOTS, c4_play, oracle_salt      # noqa: E402

SHAPES = {"m2-8": (2, 8, 11), "m4-16": (4, 16, 12), "m7-33": (7, 33, 13)}        # (m, simulations, seed)
NETS = {"stub": (0, gt.NET_STUB, 0), "hash": (10, gt.NET_HASH, oracle_salt(10))}   # (model id, the twin's net, the twin's salt)
MODES = {"fused": {}, "per-simulation": PER_SIM, "no-dedup": dict(PER_SIM, eval_dedup=0), "dedup-all": dict(PER_SIM, eval_dedup=2)}


def gumbel_off(e):
    e.selfplay_end()
    e.set_gumbel(0)          # (also puts c_visit and c_scale back at their defaults)


@pytest.fixture(autouse=True)
def gumbel_off_afterwards(engine):
    """The session's engine is shared with every other module: leave it as it was found (feature_gpu.restore does not know the new keys)."""
    yield
    gumbel_off(engine)
    fg.restore(engine)


@pytest.fixture(scope="module")
def engine3(engine_mod):
    """The seam's second game (AZ_GAME_CONNECT_THREE)."""
    yield from fg.connect_three_engine(engine_mod)


def check_conditions(ctr, exploring=True):
    """Conditions, not measurements: the parity above compared Gumbel moves, not a search that never met one."""
    print(ctr)
    assert ctr["no_considered"] == 0 and ctr["bad_schedule"] == 0, ctr
    assert ctr["root_sel"] > 0 and ctr["root_not_puct"] >= 0.25 * ctr["root_sel"], ctr
    assert ctr["moves"] > 0 and ctr["moves_not_most_visited"] >= 1 and ctr["moves_reused"] >= 0.5 * ctr["moves"], ctr
    if exploring:
        assert 0 < ctr["moves_g_zero"] < ctr["moves"], ctr


def gumbel_selfplay(e, sims, m, seed, c_visit=50.0, c_scale=1.0, **kw):
    e.set_gumbel(m, c_visit, c_scale)
    return fg.run_selfplay(e, sims, seed, **kw)


# ---- options and refusals -----------------------------------------------------------------------------------------------------------------
def test_option_ranges_and_open_session(engine, engine_mod):
    fg.check_option_ranges(engine, engine_mod,
                           bad=(("gumbel_m", (-1, 1, 8, 1 << 40)), ("gumbel_c_visit_e6", (-1, 1000000001)), ("gumbel_c_scale_e6", (-1, 0, 100000001))),
                           good=(("gumbel_m", (0, 2, 7, 4)), ("gumbel_c_visit_e6", (0, 1000000000, 50000000)), ("gumbel_c_scale_e6", (1, 100000000, 1000000))),
                           settle=lambda: engine.set_gumbel(0),
                           locked=(("gumbel_m", 4), ("gumbel_m", 0), ("gumbel_c_visit_e6", 1000000), ("gumbel_c_scale_e6", 2000000)),
                           reopen=("gumbel_m", 4))


def refused(engine_mod, call):
    with pytest.raises(engine_mod.AzError) as ei:
        call()
    assert ei.value.status == AZ_ERR_BAD_ARGUMENT


def test_refusals(engine, engine_mod):
    """num_sim_threads > 1, "selfplay_async" and forced playouts are refused while gumbel_m > 0, by every entry a Gumbel move can come from."""
    sp = dict(n_games=4, num_sims=16, model_id=10, seed=1)
    tb2 = engine.tree_create(2, reserve=gt.default_reserve(16), num_sims=16, max_depth=1000, model_id=10, cpuct=1, num_threads=2)
    tb1 = engine.tree_create(2, reserve=gt.default_reserve(16), num_sims=16, max_depth=1000, model_id=10, cpuct=1)
    states = np.zeros((2, 2), np.uint64)
    try:
        engine.set_gumbel(4)
        refused(engine_mod, lambda: engine.selfplay(num_sim_threads=2, **sp))
        refused(engine_mod, lambda: engine.selfplay_begin(4, 16, 10, seed=1, num_sim_threads=2))
        refused(engine_mod, lambda: tb2.get_action_prob(states, 1.0))
        for key, value, back in (("selfplay_async", 1, 0), ("forced_playouts_k_e6", 2000000, 0)):
            engine.set_option(key, value)
            refused(engine_mod, lambda: engine.selfplay(**sp))
            refused(engine_mod, lambda: engine.selfplay_begin(4, 16, 10, seed=1))
            refused(engine_mod, lambda: tb1.get_action_prob(states, 1.0))
            engine.set_option(key, back)
        assert engine.selfplay(**sp)["count"] > 0                  # and accepted without them
        tb1.get_action_prob(states, 1.0)
        engine.set_gumbel(0)
        for key, value, back in (("selfplay_async", 1, 0), ("forced_playouts_k_e6", 2000000, 0)):      # with the option off nothing is refused
            engine.set_option(key, value)
            assert engine.selfplay(**sp)["count"] > 0
            engine.set_option(key, back)
        tb2.get_action_prob(states, 1.0)
    finally:
        engine.selfplay_end()
        tb1.close()
        tb2.close()


# ---- the variates alone ---------------------------------------------------------------------------------------------------------------------------
def test_gumbel_values_against_the_host_build(engine):
    rng = np.random.default_rng(3)
    states, s = [], (0, 0)
    for i in range(300):                       # random positions, full columns among them
        states.append(s)
        valid = [a for a in range(7) if not ((s[0] | s[1]) >> (a * 7 + 5)) & 1]
        s = c4_play(s[0], s[1], int(rng.choice(valid))) if valid and i % 30 != 29 else (0, 0)
    states = np.array(states, np.uint64)
    ids = rng.integers(0, 1 << 40, len(states)).astype(np.uint64)
    for zero in (False, True):
        got = engine.gumbel_values(states, ids, seed=77, temp_is_zero=zero)
        want = gt.values(states, ids, seed=77, temp_is_zero=zero)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got != 0).any() != zero
    full = np.array([[(int(a) | int(b)) >> (c * 7 + 5) & 1 for c in range(7)] for a, b in states], bool)
    assert full.any() and (engine.gumbel_values(states, ids, seed=77)[full] == 0).all()


# ---- self-play parity against the twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_selfplay_parity(engine, shape, net, mode):
    m, sims, seed = SHAPES[shape]
    model_id, kind, salt = NETS[net]
    got = gumbel_selfplay(engine, sims, m, seed, model_id=model_id, options=MODES[mode])
    ref = gt.selfplay(N_GAMES, sims, m, net_kind=kind, salt=salt, seed=seed, first_game_id=1000)
    fg.check_samples_against_twin(got, ref)
    check_conditions(ref["ctr"])
    if net == "hash" and m == 4:
        assert ref["ctr"]["moves_relinked"] >= 10        # the baseline repair of a placeholder that becomes a link


def test_selfplay_parity_other_constants(engine):
    """c_visit and c_scale reach the kernels: other values, other games, still the twin's."""
    got = gumbel_selfplay(engine, 16, 4, 12, c_visit=12.5, c_scale=0.1, options=PER_SIM)
    ref = gt.selfplay(N_GAMES, 16, 4, c_visit=12.5, c_scale=0.1, net_kind=gt.NET_HASH, salt=oracle_salt(10), seed=12, first_game_id=1000)
    fg.check_samples_against_twin(got, ref)
    check_conditions(ref["ctr"])
    default = gt.selfplay(N_GAMES, 16, 4, net_kind=gt.NET_HASH, salt=oracle_salt(10), seed=12, first_game_id=1000)
    assert not np.array_equal(default["moves"], ref["moves"])


@pytest.mark.parametrize("mode", ["fused", "per-simulation"])
def test_selfplay_parity_connect_three(engine3, mode):
    try:
        got = gumbel_selfplay(engine3, 16, 4, 12, options=MODES[mode])
        ref = gt.selfplay(N_GAMES, 16, 4, net_kind=gt.NET_HASH, salt=oracle_salt(10), seed=12, first_game_id=1000, game_kind=gt.GAME_CONNECT3)
        fg.check_samples_against_twin(got, ref)
        check_conditions(ref["ctr"])
    finally:
        gumbel_off(engine3)
        fg.restore(engine3)


@pytest.mark.parametrize("mode", ["fused", "per-simulation", "dedup-all"])
def test_composition_with_root_noise_and_playout_cap(engine, mode):
    """Root noise 0.25 + playout cap (16, 5, P = 0.5) + Gumbel: full moves are Gumbel moves on the noised priors, fast moves are PUCT's."""
    got = gumbel_selfplay(engine, 16, 4, 12, options=MODES[mode], cap=(5, 500000), noise=(0.25, 0.3))
    kw = dict(net_kind=gt.NET_HASH, salt=oracle_salt(10), seed=12, first_game_id=1000, cap_sims=5, full_e6=500000, eps=0.25, alpha=0.3)
    ref = gt.selfplay(N_GAMES, 16, 4, **kw)
    fg.check_samples_against_twin(got, ref)
    check_conditions(ref["ctr"])
    full, plies = sum(bin(int(x)).count("1") for x in ref["full_masks"]), int(ref["game_len"].sum())
    assert 0.1 <= full / plies <= 0.9
    assert ref["ctr"]["moves"] == full and ref["ctr"]["root_sel"] == 16 * full          # only the full moves were Gumbel moves
    quiet = gt.selfplay(N_GAMES, 16, 4, **dict(kw, eps=0.0))
    assert not np.array_equal(quiet["pis"][:200], ref["pis"][:200])                      # the noise really entered the logits


def test_session_in_chunks_equals_one_call(engine):
    m, sims, seed = SHAPES["m7-33"]
    one = gumbel_selfplay(engine, sims, m, seed, options=PER_SIM)
    ref = gt.selfplay(N_GAMES, sims, m, net_kind=gt.NET_HASH, salt=oracle_salt(10), seed=seed, first_game_id=1000)
    fg.check_samples_against_twin(one, ref)
    fg.check_session_in_chunks(engine, one, ((0, 30), (30, 30), (60, 40)),
                               dict(n_games=N_GAMES, num_sims=sims, model_id=10, seed=seed, first_game_id=1000, concurrent=SLOTS))


# ---- conv-net replay parity -------------------------------------------------------------------------------------------------------------------------
def test_conv_net_replay_parity(engine_mod):
    """Self-play with the conv net (C = 128) and record_evals; the log is fed to the twin's ReplayNet, which must consume every record of
    every episode exactly."""
    e = engine_mod.Engine(device=0, max_batch=64, net_channels=128)
    try:
        e.net_init_random(0, seed=3)
        m, sims, seed = SHAPES["m4-16"]
        cap = 42 * (sims + 1) + 8
        got = gumbel_selfplay(e, sims, m, seed, model_id=0, record_evals=cap)
        cnt, states, pis, vs = e.selfplay_get_evals(N_GAMES, cap)
        assert (cnt > 0).all() and (cnt < cap).all()
        ref = gt.selfplay(N_GAMES, sims, m, net_kind=gt.NET_REPLAY, seed=seed, first_game_id=1000, replay=fg.flatten_eval_log(cnt, states, pis, vs))
        assert not ref["replay_bad"].any()
        fg.check_samples_against_twin(got, ref)
        check_conditions(ref["ctr"])
        st = got["stats"]
        assert st["leaf_rows_requested"] == st["leaf_rows_executed"] + st["eval_cache_hits"] + st["eval_batch_dups"], st
    finally:
        e.close()


# ---- tree calls ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [1.0, 0.0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tree_call_parity(engine, shape, temp):
    """az_tree_get_action_prob on 40 trees: twice on the same roots (the second call's root is reused: its baseline is the first call's
    visits), then on the position after the selected action: pi, counts, q and az_tree_get_selected."""
    m, sims, seed = SHAPES[shape]
    G = 40
    tb = engine.tree_create(G, reserve=gt.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=10, cpuct=1)
    twins = [gt.Tree(sims, net_kind=gt.NET_HASH, salt=oracle_salt(10)) for _ in range(G)]
    try:
        states = np.zeros((G, 2), np.uint64)
        assert (tb.selected() == -1).all()
        engine.set_gumbel(m)
        for call in range(3):
            pi, counts, q = tb.get_action_prob(states, temp, seed=seed, first_game_id=40)
            sel = tb.selected()
            for g in range(G):
                rpi, rc, rq, rsel, d = twins[g].get_action_prob(int(states[g, 0]), int(states[g, 1]), temp, seed, 40 + g, m=m)
                assert np.array_equal(counts[g], rc), (call, g, counts[g], rc)                      # raw
                assert np.array_equal(q[g].view(np.uint32), rq.view(np.uint32)), (call, g)
                assert np.array_equal(pi[g].view(np.uint32), rpi.view(np.uint32)), (call, g, pi[g], rpi)
                assert sel[g] == rsel, (call, g, sel[g], rsel)
            assert (counts.sum(axis=1) == sims * (2 if call == 1 else 1)).all() or call == 2
            assert np.allclose(pi.sum(axis=1), 1.0, atol=1e-6)
            if call == 1:
                states = np.array([c4_play(int(s[0]), int(s[1]), int(a)) for s, a in zip(states, sel)], np.uint64)
        ctr = {}
        for t in twins:
            ctr = gt.add_counters(ctr, gt.counters(t.ctr))
        print(ctr)
        assert ctr["no_considered"] == 0 and ctr["bad_schedule"] == 0 and ctr["moves"] == 3 * G and ctr["moves_reused"] >= 2 * G, ctr
        assert ctr["root_not_puct"] >= 0.25 * ctr["root_sel"] and ctr["moves_g_zero"] == (3 * G if temp == 0.0 else 0), ctr
        engine.set_gumbel(0)                    # a call that is not a Gumbel move: no selected action
        tb.get_action_prob(states, temp, seed=seed, first_game_id=40)
        assert (tb.selected() == -1).all()
    finally:
        tb.close()
        for t in twins:
            t.close()


SMALL = {"fused_search": 0, "search_graph": 4}      # per-simulation launches, four steps per captured graph: 16 simulations = four replays


def c4_over(mine, theirs):
    """The position is finished: the side that just moved (`theirs`) has four in a row, or the board is full."""
    for d in (1, 6, 7, 8):
        x = theirs & (theirs >> d)
        if x & (x >> 2 * d):
            return True
    return bin(mine | theirs).count("1") == 42


def test_tree_call_parity_with_root_noise(engine):
    """Root noise 0.25 (default alpha) and gumbel_m 4 together on az_tree_get_action_prob: both consumers of a tree's one RNG stream in the
    same call, through captured graphs.  8 trees play a whole game each, one call per ply (exploring variates on the first 6 plies, greedy
    behind them; a finished game searches its last position again): pi, counts, q and the selected action are the twin's, bit for bit."""
    sims, m, seed, G = 16, 4, 12, 8
    for k, v in SMALL.items():
        engine.set_option(k, v)
    tb = engine.tree_create(G, reserve=gt.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=10, cpuct=1)
    twins = [gt.Tree(sims, net_kind=gt.NET_HASH, salt=oracle_salt(10)) for _ in range(G + 1)]
    try:
        engine.set_root_noise(0.25)
        engine.set_gumbel(m)
        states, done, calls = np.zeros((G, 2), np.uint64), [False] * G, 0
        for ply in range(42):
            temp = 1.0 if ply < 6 else 0.0
            pi, counts, q = tb.get_action_prob(states, temp, seed=seed, first_game_id=40)
            sel = tb.selected()
            calls += 1
            for g in range(G):
                rpi, rc, rq, rsel, d = twins[g].get_action_prob(int(states[g, 0]), int(states[g, 1]), temp, seed, 40 + g, m=m, eps=0.25, alpha=1.0)
                assert np.array_equal(counts[g], rc), (ply, g, counts[g], rc)
                assert np.array_equal(q[g].view(np.uint32), rq.view(np.uint32)), (ply, g)
                assert np.array_equal(pi[g].view(np.uint32), rpi.view(np.uint32)), (ply, g, pi[g], rpi)
                assert sel[g] == rsel, (ply, g, sel[g], rsel)
                if ply == 0 and g == 0:           # the noise really entered: the same call without it gives another policy
                    qpi = twins[G].get_action_prob(0, 0, temp, seed, 40, m=m)[0]
                    assert not np.array_equal(qpi, rpi)
                if not done[g]:
                    nxt = c4_play(int(states[g, 0]), int(states[g, 1]), int(sel[g]))
                    if c4_over(*nxt):
                        done[g] = True
                    else:
                        states[g] = nxt
            if all(done):
                break
        ctr = {}
        for t in twins[:G]:
            ctr = gt.add_counters(ctr, gt.counters(t.ctr))
        print(calls, ctr)
        assert all(done) and calls > 6
        assert ctr["no_considered"] == 0 and ctr["bad_schedule"] == 0 and ctr["moves"] == calls * G, ctr
        assert ctr["root_not_puct"] >= 0.25 * ctr["root_sel"] and 0 < ctr["moves_g_zero"] < ctr["moves"], ctr
    finally:
        engine.set_option("search_graph", 20)
        tb.close()
        for t in twins:
            t.close()


def test_the_root_move_record_does_not_outlive_its_call(engine_mod):
    """Engine A runs tree calls and a self-play with root noise and gumbel_m on, then sets both to 0; engine B never sets them.  The same
    calls on both -- six tree calls on a re-rooted batch, one az_selfplay on the pooled arena A used with the keys on -- agree bit for bit."""
    sims, G = 16, 8
    sp = dict(n_games=G, num_sims=sims, model_id=10, seed=5, first_game_id=1000, concurrent=G)
    eng, tbs = [], []
    try:
        for _ in range(2):
            e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
            eng.append(e)
            e.net_set_kind(10, engine_mod.NET_HASH, HASH_SALT)
            for k, v in SMALL.items():
                e.set_option(k, v)
            tbs.append(e.tree_create(G, reserve=gt.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=10, cpuct=1))
        a, b = eng
        a.set_root_noise(0.25)
        a.set_gumbel(4)
        zeros = np.zeros((G, 2), np.uint64)
        for _ in range(2):
            tbs[0].get_action_prob(zeros, 1.0, seed=3, first_game_id=40)
        assert (tbs[0].selected() >= 0).all()                       # they were Gumbel moves
        a.set_option("root_noise_eps_e6", 0)
        a.set_option("gumbel_m", 0)
        tbs[0].reset()
        st = [zeros.copy(), zeros.copy()]
        for call in range(6):
            outs = [tb.get_action_prob(s, 1.0 if call < 4 else 0.0, seed=3, first_game_id=40) for tb, s in zip(tbs, st)]
            for x, y in zip(*outs):                                 # pi, counts, q
                assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), call
            assert (tbs[0].selected() == -1).all() and (tbs[1].selected() == -1).all()
            st = [np.array([c4_play(int(r[0]), int(r[1]), int(np.argmax(c))) for r, c in zip(s, o[1])], np.uint64) for s, o in zip(st, outs)]
        assert (outs[0][1].sum(axis=1) > 0).all()
        # through the pool: the arena of A's first az_selfplay (keys on) serves its second one (keys off)
        a.set_root_noise(0.25)
        a.set_gumbel(4)
        keys = ("count", "game_len", "moves", "states", "boards", "pis", "zs")
        on = a.selfplay(**sp)
        a.set_option("root_noise_eps_e6", 0)
        a.set_option("gumbel_m", 0)
        allocs = a.stats()["tree_arena_allocs"]
        off_a = a.selfplay(**sp)
        assert a.stats()["tree_arena_allocs"] == allocs             # the pooled arena was reused
        off_b = b.selfplay(**sp)
        fg.assert_same_outputs([off_a[k] for k in keys], [off_b[k] for k in keys])
        assert not np.array_equal(on["moves"], off_a["moves"])      # the keys really changed the games while they were on
    finally:
        for tb in tbs:
            tb.close()
        for e in eng:
            e.close()


# ---- off is off, and the arena never sees it --------------------------------------------------------------------------------------------------------------
def _plain_outputs(e):
    e.reset_stats()
    got = e.selfplay(n_games=N_GAMES, num_sims=16, model_id=10, seed=11, first_game_id=1000, concurrent=SLOTS)
    out = [got[k] for k in ("count", "game_len", "moves", "states", "boards", "pis", "zs")] + fg.arena_outputs(e)
    st = e.stats()
    return out, {k: st[k] for k in COUNTERS}


def test_off_is_off_and_the_arena_ignores_the_keys(engine_mod):
    """A fresh engine against one on which the option was on (a Gumbel self-play, then an arena with the keys still set) and is set back to
    0: az_selfplay and az_arena give the same bytes and counters."""
    res = []
    for touch in (False, True):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
        try:
            e.net_set_kind(10, engine_mod.NET_HASH, HASH_SALT)
            e.net_set_kind(11, engine_mod.NET_HASH, HASH_SALT)
            arena_on = None
            if touch:
                on = gumbel_selfplay(e, 16, 4, 11, c_visit=12.5, c_scale=2.0)
                arena_on = fg.arena_outputs(e)                       # the keys are set: the arena is what it is without them
                e.set_option("gumbel_m", 0)                          # (c_visit / c_scale stay at their odd values: inert)
            out, st = _plain_outputs(e)
            if touch:
                assert not np.array_equal(on["moves"], out[2])       # the option really changed the games while it was on
                fg.assert_same_outputs(arena_on, out[7:])
            res.append((out, st))
        finally:
            e.close()
    fg.assert_same_outputs(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]
