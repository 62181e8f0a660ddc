"""The opt-in "eval_mirror" on the GPU (include/az_engine.h): every forward of a conv model answers with F -- the net on the canonical
orientation c(s) of the position, pi un-mirrored -- on every path, a position and its mirror image share one batch row and one cache
entry, and nothing changes while the option is 0.  Every replay check feeds the engine's recorded rows to the unchanged oracle."""
import threading

import numpy as np
import pytest

import feature_gpu as fg
import mirror_twin as mt

pytestmark = pytest.mark.gpu
C = 256
KEYS = ("moves", "game_len", "pis", "zs", "states")


@pytest.fixture(scope="module")
def eng(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=1024, net_channels=C)
    e.net_init_random(0, seed=3)
    e.net_init_random(1, seed=4)
    yield e
    e.close()


@pytest.fixture()
def mirror_on(eng):
    eng.set_eval_mirror(True)
    yield eng
    eng.set_eval_mirror(False)


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def _stack(cols):
    mine = theirs = 0
    for c, col in enumerate(cols):
        for r, ch in enumerate(col):
            if ch == "x":
                mine |= 1 << (c * 7 + r)
            else:
                theirs |= 1 << (c * 7 + r)
    return mine, theirs


SYMMETRIC = [_stack(["", "", "", "x", "", "", ""]), _stack(["o", "", "", "x", "", "", "o"]), _stack(["x", "o", "", "", "", "o", "x"]),
             _stack(["", "", "xo", "ox", "xo", "", ""]), _stack(["xoxox", "", "", "", "", "", "xoxox"]),
             _stack(["x", "o", "x", "oxo", "x", "o", "x"]), _stack(["", "ox", "", "xoxox", "", "ox", ""]),
             _stack(["xo", "xo", "ox", "", "ox", "xo", "xo"])]


@pytest.fixture(scope="module")
def positions(oracle):
    """512 legal positions of mixed ply, the empty board and 8 self-symmetric positions"""
    rng = np.random.default_rng(21)
    out = []
    while len(out) < 512:
        s = (0, 0)
        for _ in range(int(rng.integers(1, 36))):
            vm = oracle.c4_valid_mask(*s)
            nxt = oracle.c4_play(s[0], s[1], int(rng.choice([a for a in range(7) if (vm >> a) & 1])))
            if oracle.c4_ended(*nxt) != 0.0:
                break
            s = nxt
        out.append(s)
    return np.array(out + [(0, 0)] + SYMMETRIC, np.uint64)


def _replay_selfplay(oracle, got, logs, n, sims, seed, sim_threads=1, game_kind=None):
    kw = {} if game_kind is None else {"game_kind": game_kind}
    ref = oracle.selfplay(n, sims, net_kind=oracle.NET_REPLAY, seed=seed, threads=16, sim_threads=sim_threads,
                          replay=fg.flatten_eval_log(*logs), **kw)
    assert not ref["replay_bad"].any(), np.flatnonzero(ref["replay_bad"])[:5]
    assert np.array_equal(ref["moves"], got["moves"]) and np.array_equal(ref["game_len"], got["game_len"])
    assert np.array_equal(ref["pis"], got["pis"]) and np.array_equal(ref["zs"], got["zs"])


# ---- 1. the function --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("klass", ["bf16", "fp8"])
def test_the_function(eng, engine_mod, oracle, positions, klass):
    """F(mirror s) is F(s) with pi reversed and equal v, and F(s) is the option-OFF row of c(s) un-mirrored by the twin, as bytes, at batch
    sizes 1, 33 and the whole set, in both numerics classes; az_net_predict on the feature planes agrees.  A self-symmetric position IS
    its own mirror image (c(s) = s, not mirrored), so there F(mirror s) is F(s) itself -- pi of a conv net is not symmetric, and the
    contract does not make it so."""
    if klass == "fp8":
        eng.net_set_class(0, engine_mod.NET_CLASS_FP8)
    try:
        mir = mt.mirror_batch(positions)
        sym = np.all(mir == positions, axis=1)
        assert int(sym.sum()) >= 9 and int((~sym).sum()) >= 400
        off_c = eng.predict_states(mt.canonical_batch(positions)[0], 0)
        raw = eng.predict_states(positions, 0)
        eng.set_eval_mirror(True)
        for n in (1, 33, len(positions)):
            for lo in ((0, 200, len(positions) - 1) if n == 1 else (0, len(positions) - n)):
                s = positions[lo:lo + n]
                pi, v = eng.predict_states(s, 0)
                pim, vm = eng.predict_states(mir[lo:lo + n], 0)
                k = sym[lo:lo + n]
                assert same((pim[~k], pim[k], vm), (pi[~k][:, ::-1], pi[k], v)), (n, lo)
                want = mt.f_from_n(lambda c: (off_c[0][lo:lo + n], off_c[1][lo:lo + n]), s)
                assert same((pi, v), want), (n, lo)
                pb, vb = eng.predict(mt.states_to_boards(s), 0)
                assert same((pb, vb), (pi, v)), (n, lo)
        f_all = eng.predict_states(positions, 0)
        assert not same(f_all, raw)                        # the net is not equivariant: F is another function
        flags = mt.canonical_batch(positions)[1].astype(bool)
        assert same((f_all[0][~flags], f_all[1][~flags]), (raw[0][~flags], raw[1][~flags]))
    finally:
        eng.set_eval_mirror(False)
        if klass == "fp8":
            eng.net_set_class(0, engine_mod.NET_CLASS_ENGINE)


# ---- 2. self-play and the row count ---------------------------------------------------------------------------------------------------
def test_selfplay_replays_and_executes_fewer_rows_than_distinct_states(mirror_on, oracle):
    """1024 games x 25 sims on 256 slots (slot refill): every episode replays on the oracle, the logged rows are F of their states, and the
    net ran on FEWER rows than the log holds distinct states -- impossible with the option off, where every distinct state is executed at
    least once per call -- and on at least as many as it holds distinct canonical states."""
    e = mirror_on
    n, sims, seed = 1024, 25, 5
    cap = 42 * (sims + 1) + 8
    e.reset_stats()
    got = e.selfplay(n_games=n, num_sims=sims, model_id=0, seed=seed, concurrent=256, record_evals=cap, want_boards=False)
    st = e.stats()
    logs = e.selfplay_get_evals(n, cap)
    assert logs[0].max() <= cap and logs[0].min() > 0
    _replay_selfplay(oracle, got, logs, n, sims, seed)
    _, fs, fp, fv = fg.flatten_eval_log(*logs)
    keys, first, inv = np.unique(mt.pack_batch(fs), return_index=True, return_inverse=True)
    upi, uv = e.predict_states(fs[first], 0)
    assert same((upi[inv], uv[inv]), (fp, fv))
    distinct = len(keys)
    canon = len(np.unique(mt.pack_batch(mt.canonical_batch(fs[first])[0])))
    print(f"eval_mirror self-play {n} x {sims}: requested {st['leaf_rows_requested']} executed {st['leaf_rows_executed']} "
          f"cache hits {st['eval_cache_hits']} batch dups {st['eval_batch_dups']}; distinct states in the log {distinct}, canonical {canon}")
    assert st["leaf_rows_requested"] == st["leaf_evals"] == len(fv)
    assert st["leaf_rows_requested"] == st["leaf_rows_executed"] + st["eval_cache_hits"] + st["eval_batch_dups"]
    assert canon <= st["leaf_rows_executed"] < distinct, (canon, st["leaf_rows_executed"], distinct)


# ---- 3. F does not depend on de-duplication ---------------------------------------------------------------------------------------------
def test_f_does_not_depend_on_dedup(mirror_on):
    e = mirror_on
    runs = {}
    try:
        for mode in (0, 1):
            e.set_option("eval_dedup", mode)
            e.reset_stats()
            runs[mode] = (e.selfplay(n_games=128, num_sims=25, model_id=0, seed=8, concurrent=64), e.stats())
    finally:
        e.set_option("eval_dedup", 1)
    for k in KEYS:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
    assert runs[0][1]["leaf_rows_executed"] == runs[0][1]["leaf_rows_requested"] == runs[1][1]["leaf_rows_requested"]
    assert runs[1][1]["leaf_rows_executed"] < runs[1][1]["leaf_rows_requested"]


# ---- 4. every schedule ------------------------------------------------------------------------------------------------------------------
def test_every_schedule(mirror_on, oracle):
    """One-shot, a session fetched in chunks of 64 and the free-running driver give the same tuples; four simulations in flight replay on
    the oracle's lock-step search."""
    e = mirror_on
    n, sims, seed = 256, 24, 31
    cap = 42 * (sims + 1) + 8
    ref = e.selfplay(n_games=n, num_sims=sims, model_id=0, seed=seed, concurrent=96, want_boards=False, record_evals=cap)
    _replay_selfplay(oracle, ref, e.selfplay_get_evals(n, cap), n, sims, seed)
    e.selfplay_begin(n, sims, 0, seed=seed, concurrent=96)
    with pytest.raises(Exception) as ei:                          # refused while the session is open
        e.set_option("eval_mirror", 0)
    assert getattr(ei.value, "status", None) == 1
    parts = [e.selfplay_next(64, want_boards=False) for _ in range(4)]
    e.selfplay_end()
    for k in KEYS:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), ref[k]), k
    try:
        e.set_option("selfplay_async", 1)
        got = e.selfplay(n_games=n, num_sims=sims, model_id=0, seed=seed, concurrent=96, want_boards=False)
    finally:
        e.set_option("selfplay_async", 0)
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), k
    mt4 = e.selfplay(n_games=n, num_sims=sims, model_id=0, seed=seed, concurrent=96, want_boards=False, record_evals=cap, num_sim_threads=4)
    _replay_selfplay(oracle, mt4, e.selfplay_get_evals(n, cap), n, sims, seed, sim_threads=4)


# ---- 5. tree calls ----------------------------------------------------------------------------------------------------------------------
def _replay_tree(oracle, sims, log, g, hist, seed):
    cnt, lstates, lpis, lvs = log
    t = oracle.Tree(sims, net_kind=oracle.NET_REPLAY)
    t.set_replay(lstates[g, :cnt[g]], lpis[g, :cnt[g]], lvs[g, :cnt[g]])
    for sts, pi, counts, q in hist:
        opi, ocnt, oq = t.get_action_prob(sts[g][0], sts[g][1], 1.0, seed=seed, game_id=g)
        assert np.array_equal(counts[g], ocnt) and np.array_equal(pi[g], opi) and np.array_equal(q[g], oq), g
    assert not t.replay_bad()
    t.close()


def _tree_moves(e, oracle, G, sims, moves, seed, model_id=0):
    tb = e.tree_create(G, reserve=oracle.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=model_id, cpuct=1)
    tb.record_evals(moves * (sims + 1) + 8)
    states, hist = [(0, 0)] * G, []
    rng = np.random.default_rng(2)
    for _ in range(moves):
        pi, counts, q = tb.get_action_prob(np.array(states, dtype=np.uint64), 1.0, seed=seed)
        hist.append((list(states), pi, counts, q))
        states = [oracle.c4_play(s[0], s[1], int(rng.choice([a for a in range(7) if pi[g][a] > 0]))) for g, s in enumerate(states)]
    log = tb.get_evals()
    tb.close()
    return hist, log


def test_tree_get_action_prob_replays(mirror_on, oracle):
    G, sims = 12, 100
    hist, log = _tree_moves(mirror_on, oracle, G, sims, 6, seed=4)
    for g in range(G):
        _replay_tree(oracle, sims, log, g, hist, 4)
    fs = np.concatenate([log[1][g, :log[0][g]] for g in range(G)])
    assert (mt.canonical_batch(fs)[1] == 1).any() and (mt.canonical_batch(fs)[1] == 0).any()


def test_shared_tree_batch(mirror_on, oracle):
    """4 host threads on 4 slots, 25 sims, three moves each: every answer is the 1-game tree's, bit for bit."""
    e = mirror_on
    sims, seed = 25, 6
    tb = e.tree_create(4, reserve=oracle.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=0, cpuct=1)
    tb.share(200)
    answers, errors = {}, []

    def worker(i):
        try:
            slot = tb.slot_acquire()
            s, out = (0, 0), []
            for a in (i % 7, (2 * i + 3) % 7):                    # four different openings, one of them and its mirror image among them
                s = oracle.c4_play(s[0], s[1], a)
            for _ in range(3):
                pi, counts, q = tb.slot_get_action_prob(slot, s, 1.0, seed=seed, game_id=100 + i)
                out.append((s, pi, counts, q))
                s = oracle.c4_play(s[0], s[1], int(np.argmax(counts)))
            tb.slot_release(slot)
            answers[i] = out
        except Exception as ex:             # noqa: BLE001
            errors.append((i, repr(ex)))
    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    tb.close()
    assert not errors, errors
    for i in range(4):
        one = e.tree_create(1, reserve=oracle.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=0, cpuct=1)
        for s, pi, counts, q in answers[i]:
            got = one.get_action_prob(np.array([s], np.uint64), 1.0, seed=seed, first_game_id=100 + i)
            assert same((got[0][0], got[1][0], got[2][0]), (pi, counts, q)), i
        one.close()


# ---- 6. arena ---------------------------------------------------------------------------------------------------------------------------
def test_arena_replays_for_both_players(mirror_on, oracle):
    e = mirror_on
    num, sims = 64, 25
    cap = 22 * (sims + 1) + 8
    wld, res = e.arena(num, sims, new_model_id=1, old_model_id=0, seed=9, record_evals=cap)
    logs = [e.arena_get_evals(w, num, cap) for w in (0, 1)]
    rn, ro = (fg.flatten_eval_log(*logs[w]) for w in (0, 1))
    owld, ores, bad = oracle.arena_ex(num, sims, first_game=0, n_games=num, net_kind=oracle.NET_REPLAY, seed=9, threads=16,
                                      replay_new=rn, replay_old=ro)
    assert not bad.any() and np.array_equal(ores, res) and owld.tolist() == wld.tolist() and int(wld.sum()) == num
    for w, mid in ((0, 1), (1, 0)):
        pi2, v2 = e.predict_states(rn[1] if w == 0 else ro[1], mid)
        assert same((pi2, v2), (rn[2], rn[3]) if w == 0 else (ro[2], ro[3]))
    glen, gmoves = e.arena_get_moves(num)
    for g in range(num):                                          # the move record ends each game at its recorded result
        s, player = (0, 0), 1
        for k in range(int(glen[g])):
            assert oracle.c4_ended(*s) == 0.0
            s = oracle.c4_play(s[0], s[1], int(gmoves[g, k]))
            player = -player
        end = oracle.c4_ended(*s)
        assert end != 0.0 and int(res[g]) == (-player if end == -1.0 else (player if end == 1.0 else 0)), g


# ---- 7. class hygiene -------------------------------------------------------------------------------------------------------------------
def test_no_cached_row_crosses_the_class(engine_mod):
    def fresh():
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=C)
        e.net_init_random(0, seed=3)
        e.set_option("eval_cache_persist", 1)
        e.set_option("eval_cache_log2", 20)
        return e
    a, b = fresh(), fresh()
    try:
        a.set_eval_mirror(True)
        on = a.selfplay(n_games=64, num_sims=25, model_id=0, seed=2)
        a.set_eval_mirror(False)
        a.reset_stats()
        off = a.selfplay(n_games=64, num_sims=25, model_id=0, seed=2)
        sa = a.stats()
        b.reset_stats()
        ref = b.selfplay(n_games=64, num_sims=25, model_id=0, seed=2)
        sb = b.stats()
        for k in KEYS + ("boards",):
            assert np.array_equal(off[k], ref[k]), k
        # ... and not by luck: a leaked canonical row would hold the right value for the canonical half of the states (N(c(s)) IS N(s)
        # there), so the outputs alone cannot show a leak -- the row count does.  About half of the off run's distinct states are their
        # own canonical form and would hit at once, a cut of the executed rows by tens of per cent; what may differ without a leak is
        # the odd row that one run's lookup finds published a launch earlier than the other's
        assert sa["leaf_rows_requested"] == sb["leaf_rows_requested"]
        print("off run behind a mirror run: executed", sa["leaf_rows_executed"], "fresh engine:", sb["leaf_rows_executed"])
        assert sa["leaf_rows_executed"] >= 0.9 * sb["leaf_rows_executed"], (sa["leaf_rows_executed"], sb["leaf_rows_executed"])
        assert not all(np.array_equal(on[k], off[k]) for k in KEYS)
    finally:
        a.close()
        b.close()


def test_no_captured_graph_crosses_the_class(eng, oracle):
    """A graph-replayed tree call (12 trees: far below "search_graph_rows") off, on, off on fresh tree batches of one shape."""
    G, sims = 12, 40
    first = _tree_moves(eng, oracle, G, sims, 2, seed=4)
    eng.set_eval_mirror(True)
    try:
        hist, log = _tree_moves(eng, oracle, G, sims, 2, seed=4)
    finally:
        eng.set_eval_mirror(False)
    third = _tree_moves(eng, oracle, G, sims, 2, seed=4)
    for (_, pa, ca, qa), (_, pb, cb, qb) in zip(first[0], third[0]):
        assert same((pa, ca, qa), (pb, cb, qb))
    assert same(first[1], third[1])
    for g in range(G):
        _replay_tree(oracle, sims, log, g, hist, 4)
    assert not same(first[1][2:], log[2:])


def test_option_values(eng):
    for bad in (2, -1):
        with pytest.raises(Exception) as ei:
            eng.set_option("eval_mirror", bad)
        assert getattr(ei.value, "status", None) == 1             # AZ_ERR_BAD_ARGUMENT
    eng.selfplay_begin(8, 25, 0, seed=1)
    try:
        for v in (1, 0):
            with pytest.raises(Exception) as ei:
                eng.set_option("eval_mirror", v)
            assert getattr(ei.value, "status", None) == 1
    finally:
        eng.selfplay_end()
    eng.set_option("eval_mirror", 0)


# ---- 8. other nets and the default ------------------------------------------------------------------------------------------------------
def test_hash_net_is_never_affected(mirror_on, engine_mod, oracle):
    e = mirror_on
    e.net_set_kind(10, engine_mod.NET_HASH, 1234)
    ref = oracle.selfplay(64, 25, net_kind=oracle.NET_HASH, salt=1234 + 10 * 0x51ED27, seed=5)
    try:
        for fused, dedup in ((1, 1), (0, 1), (1, 2)):
            e.set_option("fused_search", fused)
            e.set_option("eval_dedup", dedup)
            got = e.selfplay(n_games=64, num_sims=25, model_id=10, seed=5)
            assert np.array_equal(got["moves"], ref["moves"]) and np.array_equal(got["pis"], ref["pis"]), (fused, dedup)
            assert np.array_equal(got["zs"], ref["zs"]) and np.array_equal(got["boards"].reshape(-1, 84), ref["boards"].reshape(-1, 84))
    finally:
        e.set_option("fused_search", 1)
        e.set_option("eval_dedup", 1)


def test_option_0_is_the_engine_that_never_set_it(engine_mod):
    def run(set_it):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=C)
        try:
            e.net_init_random(0, seed=3)
            if set_it:
                e.set_option("eval_mirror", 0)
            e.reset_stats()
            return e.selfplay(n_games=64, num_sims=25, model_id=0, seed=12), e.stats()
        finally:
            e.close()
    (a, sa), (b, sb) = run(True), run(False)
    for k in KEYS + ("boards",):
        assert np.array_equal(a[k], b[k]), k
    for k in ("leaf_evals", "leaf_rows_requested", "leaf_rows_executed", "eval_cache_hits", "eval_batch_dups", "eval_cache_inserts", "simulations"):
        assert sa[k] == sb[k], k


# ---- 9. the second game -----------------------------------------------------------------------------------------------------------------
def test_connect_three_replays(engine_mod, oracle):
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=C, game=1)
    try:
        e.net_init_random(0, seed=3)
        e.set_eval_mirror(True)
        n, sims, seed = 64, 25, 14
        cap = 42 * (sims + 1) + 8
        got = e.selfplay(n_games=n, num_sims=sims, model_id=0, seed=seed, record_evals=cap, want_boards=False)
        logs = e.selfplay_get_evals(n, cap)
        _replay_selfplay(oracle, got, logs, n, sims, seed, game_kind=oracle.GAME_CONNECT3)
        _, fs, fp, fv = fg.flatten_eval_log(*logs)
        assert same(e.predict_states(fs[:512], 0), (fp[:512], fv[:512]))
        assert mt.canonical_batch(fs)[1].any()
    finally:
        e.close()


# ---- 10. the hosts ----------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_coach_agree_with_eval_mirror(engine_mod, tmp_path):
    def mirror(on):
        def configure(coach, e):
            coach.eval_mirror = on
        return configure
    fg.run_coach_pair(engine_mod, tmp_path, ["eval_mirror=1", "num_eps=64"], mirror(True), num_eps=64, plain=mirror(False))
