"""Calls interleaved with the engine's two pieces of long-lived device state -- an open self-play session (az_selfplay_begin / _next /
_end, lock-step and free-running) and the evaluation cache with its 15-bit model tags -- held to the contract of include/az_engine.h
(next to az_selfplay_begin).  tests/session_contract.py is the table: every export and every option key with its class; each row gets
one session per driver here, so a failure names its row.

The reference is never the disturbed run: for the hash nets it is the CPU oracle's execute_episode, for the conv net the one-shot
az_selfplay of a fresh engine (itself pinned by replay parity, tests/test_net_gpu.py)."""
import ctypes

import numpy as np
import pytest

import session_contract as sc

pytestmark = pytest.mark.gpu

AZ_ERR_BAD_ARGUMENT = 1
MODEL_SALT = 0x51ED27
SEED = 21
# the smallest shapes where slots refill (episodes > slots), the cache fills and a chunk ends while later episodes are in flight
HASH_SHAPE = dict(n=96, sims=25, slots=16, chunks=(32, 32, 32))
CONV_SHAPE = dict(n=48, sims=16, slots=16, chunks=(16, 16, 16))
PERSIST_LOG2 = 18                     # a persistent cache has its full configured size from the first call: 2^18 entries hold these runs
DRIVERS = (0, 1)                      # "selfplay_async": the lock-step and the free-running driver
KEYS = ("game_len", "moves", "boards", "pis", "zs")
# the rows that also run beside a CONV-net session (the net-touching ones; every row runs beside a hash-net session)
CONV_SESSION_ROWS = ("az_net_free", "az_net_set_params", "az_net_train", "az_net_predict_states", "az_net_evaluate", "az_net_get_params",
                     "conv2_table", "narrow_rows", "search_graph")


def oracle_salt(model_id):
    return sc.HASH_SALT + model_id * MODEL_SALT


def same(a, b):
    """Bit for bit, through tuples, lists and dicts."""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def chunk_of(ref, chunks, i):
    """Chunk i of a whole run: the episodes' rows and their tuples (two per ply: identity + mirror)."""
    lo = sum(chunks[:i])
    hi = lo + chunks[i]
    t0, t1 = 2 * int(ref["game_len"][:lo].sum()), 2 * int(ref["game_len"][:hi].sum())
    keys = KEYS + (("states",) if "states" in ref else ())          # the oracle has no packed states: its boards carry the positions
    return {k: (ref[k][lo:hi] if k in ("game_len", "moves") else ref[k][t0:t1]) for k in keys}


def assert_chunk(got, ref, chunks, i, what):
    want = chunk_of(ref, chunks, i)
    assert got["count"] == len(want["zs"]) == len(got["states"]), (what, i)
    for k in want:
        assert same(np.asarray(got[k]).reshape(len(want[k]), -1), np.asarray(want[k]).reshape(len(want[k]), -1)), (what, "chunk", i, k)


@pytest.fixture(scope="module")
def hash_ref(oracle):
    s = HASH_SHAPE
    return oracle.selfplay(s["n"], s["sims"], net_kind=oracle.NET_HASH, salt=oracle_salt(sc.HASH_ID), seed=SEED, threads=8)


@pytest.fixture(scope="module")
def conv_ref(engine_mod):
    s = CONV_SHAPE
    e = sc.make_engine(engine_mod, conv=True)
    try:
        return e.selfplay(n_games=s["n"], num_sims=s["sims"], model_id=sc.CONV_ID, seed=SEED, concurrent=s["slots"])
    finally:
        e.close()


def params_of(rows, classes):
    out = []
    for row in rows:
        if row.cls not in classes:
            continue
        for driver in DRIVERS:
            out.append(pytest.param(row, driver, False, id="%s-%s-hash" % (row.name, "async" if driver else "lockstep")))
            if row.name in CONV_SESSION_ROWS:
                out.append(pytest.param(row, driver, True, id="%s-%s-conv" % (row.name, "async" if driver else "lockstep")))
    return out


def open_session(engine_mod, row, driver, conv_session, tmp_path):
    e = sc.make_engine(engine_mod, conv=row.conv or conv_session)
    ctx = sc.Ctx(engine_mod, e, conv_session, tmp_path)
    if row.prep:
        row.prep(ctx)
    e.set_option("selfplay_async", driver)
    shape = CONV_SHAPE if conv_session else HASH_SHAPE
    e.selfplay_begin(shape["n"], shape["sims"], ctx.sid, seed=SEED, concurrent=shape["slots"])
    return e, ctx, shape


def stats_without_time(e):
    st = e.stats()
    st.pop("device_ms")          # wall time inside engine calls: az_selfplay_next itself moves it
    return st


@pytest.mark.parametrize("row,driver,conv_session", params_of(sc.ROWS, (sc.REFUSED, sc.BY_MODEL)))
def test_refused_rows(engine_mod, hash_ref, conv_ref, tmp_path, row, driver, conv_session):
    """Between chunk 1 and chunk 2 the call is refused with AZ_ERR_BAD_ARGUMENT and a message that names it; every counter reads as
    before; chunks 2 and 3 are the reference's.  (A BY_MODEL row names the session's model here.)"""
    ref = conv_ref if conv_session else hash_ref
    e, ctx, shape = open_session(engine_mod, row, driver, conv_session, tmp_path)
    try:
        chunks = shape["chunks"]
        assert_chunk(e.selfplay_next(chunks[0]), ref, chunks, 0, row.name)
        before = stats_without_time(e)
        with pytest.raises(engine_mod.AzError) as ei:
            if row.cls == sc.BY_MODEL:
                row.call(ctx, ctx.sid)
            else:
                row.call(ctx)
        assert ei.value.status == AZ_ERR_BAD_ARGUMENT, (row.name, str(ei.value))
        assert row.name in str(ei.value), (row.name, str(ei.value))
        assert stats_without_time(e) == before, row.name
        for i in (1, 2):
            assert_chunk(e.selfplay_next(chunks[i]), ref, chunks, i, row.name)
    finally:
        e.selfplay_end()
        e.close()


@pytest.mark.parametrize("row,driver,conv_session", params_of(sc.ROWS, (sc.INERT, sc.BY_MODEL)))
def test_inert_rows(engine_mod, hash_ref, conv_ref, tmp_path, row, driver, conv_session):
    """The call is made between chunks 1 and 2 and again between chunks 2 and 3: all three chunks are the reference's, and the call's
    own output is what the same calls return on an engine with no session open.  (A BY_MODEL row names another model id here.)"""
    ref = conv_ref if conv_session else hash_ref
    args = (sc.SCRATCH_ID,) if row.cls == sc.BY_MODEL else ()
    plain = sc.make_engine(engine_mod, conv=row.conv or conv_session)
    try:
        pctx = sc.Ctx(engine_mod, plain, conv_session, tmp_path)
        if row.prep:
            row.prep(pctx)
        want = [row.call(pctx, *args), row.call(pctx, *args)]
    finally:
        plain.close()
    e, ctx, shape = open_session(engine_mod, row, driver, conv_session, tmp_path)
    try:
        chunks = shape["chunks"]
        got = []
        for i in range(3):
            if i:
                got.append(row.call(ctx, *args))
            assert_chunk(e.selfplay_next(chunks[i]), ref, chunks, i, row.name)
        if row.compare:
            assert same(got, want), (row.name, got, want)
    finally:
        e.selfplay_end()
        e.close()


# ---- "conv2_table" and a persistent cache, no session ---------------------------------------------------------------------------------------
def test_conv2_table_retags_a_persistent_cache(engine_mod):
    """The table set and the GEMM set of conv2 round differently, so with "eval_cache_persist" 1 a change of "conv2_table" must give every
    conv model a new cache tag: self-play after the flip -- tuples AND the rows its searches consumed -- is bit for bit a fresh engine's
    at that value, in both directions."""
    s = CONV_SHAPE
    cap = 42 * (s["sims"] + 1) + 8

    def play(e):
        out = e.selfplay(n_games=s["n"], num_sims=s["sims"], model_id=sc.CONV_ID, seed=SEED, concurrent=s["slots"], record_evals=cap)
        cnt, st, pis, vs = e.selfplay_get_evals(s["n"], cap)
        rows = [np.concatenate([a[g, :cnt[g]] for g in range(s["n"])]) for a in (st, pis, vs)]
        return [out[k] for k in KEYS + ("states",)] + [cnt] + rows

    def fresh(table):
        e = sc.make_engine(engine_mod, conv=True)
        e.set_option("eval_cache_log2", PERSIST_LOG2)
        e.set_option("eval_cache_persist", 1)
        e.set_option("conv2_table", table)
        return e

    e, f = fresh(1), fresh(0)
    try:
        at1 = play(e)
        want0 = play(f)
        assert not same(at1[-1], want0[-1]), "the two sets gave the same value rows: the check below would be vacuous"
        e.set_option("conv2_table", 0)
        assert same(play(e), want0)
        e.set_option("conv2_table", 1)
        assert same(play(e), at1)
    finally:
        e.close()
        f.close()


# ---- the 15-bit tag counter wraps -----------------------------------------------------------------------------------------------------------
def _set_next_tag(e, value):
    fn = e._lib.az_diag_set_next_cache_tag
    fn.restype, fn.argtypes = ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_longlong]
    assert fn(e._h, value) >= 1


def _wrap_engine(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=sc.MAX_BATCH, net_channels=sc.CHANNELS, diag=True)
    e.set_option("eval_dedup", 2)
    e.set_option("eval_cache_log2", PERSIST_LOG2)
    e.set_option("eval_cache_persist", 1)
    for mid in (10, 11, 12):
        e.net_set_kind(mid, engine_mod.NET_HASH, sc.HASH_SALT)
    return e


def _assert_selfplay(e, oracle, mid, n=32, sims=25, seed=5):
    got = e.selfplay(n_games=n, num_sims=sims, model_id=mid, seed=seed, concurrent=16)
    ref = oracle.selfplay(n, sims, net_kind=oracle.NET_HASH, salt=oracle_salt(mid), seed=seed, threads=8)
    assert got["count"] == ref["count"]
    for k in KEYS:
        assert same(np.asarray(got[k]).reshape(len(ref[k]), -1), np.asarray(ref[k]).reshape(len(ref[k]), -1)), k


def test_tag_wrap_at_a_models_first_search(engine_mod, oracle):
    """(a) Model 11 fills the persistent cache under tag 1; the counter is put at its end; model 10's first search wraps it, clears the
    cache and takes tag 1 itself.  Its games are the oracle's, and its cache hits are those of a cold cache: not one of model 11's rows,
    filed under the same tag over the same openings, is found."""
    cold = _wrap_engine(engine_mod)
    e = _wrap_engine(engine_mod)
    try:
        _assert_selfplay(cold, oracle, 10)
        cold_hits = cold.stats()["eval_cache_hits"]
        _assert_selfplay(e, oracle, 11)
        assert e.stats()["eval_cache_inserts"] > 0
        _set_next_tag(e, 0x8000)
        e.reset_stats()
        _assert_selfplay(e, oracle, 10)
        assert e.stats()["eval_cache_hits"] == cold_hits
        _assert_selfplay(e, oracle, 11)                     # model 11 lost its tag to the wrap and gets a new one
    finally:
        cold.close()
        e.close()


def test_tag_wrap_between_the_models_of_an_arena(engine_mod, oracle):
    """(b) The last tag goes to az_arena's first model, the wrap falls on its second: the games are the oracle's play_games."""
    e = _wrap_engine(engine_mod)
    try:
        _assert_selfplay(e, oracle, 12)                     # entries from before the wrap
        _set_next_tag(e, 0x7FFF)
        wld, res = e.arena(16, 25, new_model_id=11, old_model_id=10, seed=9)
        owld, ores = oracle.arena(16, 25, net_kind=oracle.NET_HASH, salt=sc.HASH_SALT, seed=9, new_model_id=11, old_model_id=10, threads=8)
        assert same(res, ores) and wld.tolist() == owld.tolist()
        for mid in (10, 11, 12):
            _assert_selfplay(e, oracle, mid)
    finally:
        e.close()


def test_tag_wrap_inside_a_tournament(engine_mod, oracle):
    """(c) Three untagged models and two tags left: the wrap falls on the third model of az_tournament.  Every pair's games are the
    oracle's play_games of that pair."""
    e = _wrap_engine(engine_mod)
    try:
        _assert_selfplay(e, oracle, 12)
        for mid in (10, 11, 12):
            e.net_set_kind(mid, engine_mod.NET_HASH, sc.HASH_SALT)      # an upload: every tag back to none
        _set_next_tag(e, 0x7FFE)
        ids, n = (10, 11, 12), 8
        got = e.tournament(ids, n, 25, seed=9)
        p = 0
        for i in range(3):
            for j in range(i + 1, 3):
                owld, ores = oracle.arena(n, 25, net_kind=oracle.NET_HASH, salt=sc.HASH_SALT, seed=9, new_model_id=ids[i], old_model_id=ids[j], threads=8)
                assert same(got["results"][p * n:(p + 1) * n], ores), (i, j)
                assert got["wld"][i, j].tolist() == owld.tolist(), (i, j)
                p += 1
        for mid in ids:
            _assert_selfplay(e, oracle, mid)
    finally:
        e.close()


# ---- lifetime -------------------------------------------------------------------------------------------------------------------------------
def free_device_memory(engine_mod):
    """hipMemGetInfo of the HIP runtime the engine library itself is linked to (resolved through the library's own handle)."""
    hip = ctypes.CDLL(engine_mod.LIB_PATH)
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0 and total.value > 0
    return free.value


@pytest.mark.parametrize("driver", DRIVERS, ids=["lockstep", "async"])
def test_destroy_with_an_open_session_frees_everything(engine_mod, driver):
    """az_destroy with a session in flight closes it: free device memory is back at its value before az_create.  The session is sized
    so that a leak would show: 1024 resident trees of 50 simulations and the cache its 4096 episodes can fill are over a gigabyte."""
    free0 = free_device_memory(engine_mod)
    e = sc.make_engine(engine_mod, conv=False)
    e.set_option("selfplay_async", driver)
    e.selfplay_begin(4096, 50, sc.HASH_ID, seed=SEED, concurrent=1024)
    got = e.selfplay_next(8)
    assert got["count"] > 0
    held = free0 - free_device_memory(engine_mod)
    assert held > 512 << 20, held
    e.close()                                               # az_destroy, the session still open
    free1 = free_device_memory(engine_mod)
    assert abs(free0 - free1) < 64 << 20, (free0, free1, held)


# ---- an open training session ---------------------------------------------------------------------------------------------------------------
def test_training_session_rule(engine_mod):
    """While az_net_train_begin .. az_net_train_end is open, az_net_train and az_net_train_samples are refused and the session goes on
    as if they had not been called; a second az_net_train_begin is a restart, bit for bit a first begin."""
    boards = np.stack([engine_mod.c4_features(int(s[0]), int(s[1])) for s in sc.STATES]).astype(np.float32)
    other = boards[::-1].copy()

    def engine():
        e = engine_mod.Engine(device=0, max_batch=sc.MAX_BATCH, net_channels=sc.CHANNELS)
        e.net_init_random(1, seed=4)
        for key, val in (("train_epochs", 1), ("train_batch", 4)):
            e.set_option(key, val)
        return e

    def step_and_end(e, dst):
        out = e.train_step(boards, sc.PIS, sc.ZS, mask_seed=7, apply=True, want_grads=True)
        info = e.train_step_info()
        e.train_end(dst)
        return [out[0], out[1], info, e.net_get_params(dst)]

    f, e = engine(), engine()
    try:
        f.train_begin(1)
        want = step_and_end(f, 2)
        # refusals leave the open session alone
        e.train_begin(1)
        for name, call in (("az_net_train", lambda: e.train(1, 3, boards, sc.PIS, sc.ZS)),
                           ("az_net_train_samples", lambda: e.train_samples(1, 3, sc.PIS, sc.ZS, states=sc.STATES))):
            with pytest.raises(engine_mod.AzError) as ei:
                call()
            assert ei.value.status == AZ_ERR_BAD_ARGUMENT and name in str(ei.value), (name, str(ei.value))
        with pytest.raises(engine_mod.AzError):
            e.net_get_params(3)                             # ... and stored nothing
        assert same(step_and_end(e, 2), want)
        # a second begin restarts: two applied steps on other data are forgotten
        e.train_begin(1)
        for k in range(2):
            e.train_step(other, sc.PIS, sc.ZS[::-1].copy(), mask_seed=90 + k, apply=True)
        e.train_begin(1)
        assert same(step_and_end(e, 4), want)
        e.train(1, 5, boards, sc.PIS, sc.ZS)                # and with the session closed az_net_train runs
    finally:
        f.close()
        e.close()
