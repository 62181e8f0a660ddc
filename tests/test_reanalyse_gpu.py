"""az_reanalyse on the GPU (include/az_reanalyse.h): every row against the one-tree az_tree_get_action_prob that
defines it, bit for bit under every option group; root_q against the numpy restatement of csrc/az_target.h and root_prior against
az_selfplay_get_search; independence of `concurrent`, order, route, pointer kind and cache state; the refusals; the session contract
(REFUSED) and purity beside the other entry points; and the two Coaches with reanalyse_sims.

Shapes: 70 positions of a short hash-net self-play at all plies (duplicates left in), concurrent = 40 -- one whole 32-tree workgroup plus a
partial wave, then a short last chunk of 30 -- and 25 simulations, on an engine of max_batch 256 and 128 channels."""
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
from feature_gpu import AZ_ERR_BAD_ARGUMENT, HASH_SALT      # noqa: E402

AZ_ERR_CAPACITY = 2
N, CONCURRENT, SIMS = 70, 40, 25
SEED, FIRST = 5, 1000
HASH, HASH2, CONV, CONV_FP8 = 10, 11, 0, 1
OUT_KEYS = ("pi", "counts", "q", "selected", "root_q", "root_prior")
SUMMED = ("simulations", "expansions", "link_hits", "terminal_hits", "leaf_rows_requested")


@pytest.fixture(scope="module")
def eng(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    e.net_set_kind(HASH, engine_mod.NET_HASH, HASH_SALT)
    e.net_set_kind(HASH2, engine_mod.NET_HASH, HASH_SALT)
    e.net_init_random(CONV, seed=3)
    e.net_init_random(CONV_FP8, seed=3)
    e.net_set_class(CONV_FP8, engine_mod.NET_CLASS_FP8)
    yield e
    e.close()


def set_options(e, opts):
    """The option groups a row names; everything it does not name is at the engine's default."""
    fg.restore(e)
    e.set_gumbel(0)
    e.set_eval_mirror(False)
    for k, v in opts.get("options", {}).items():
        e.set_option(k, v)
    if "noise" in opts:
        e.set_root_noise(*opts["noise"])
    if "forced" in opts:
        e.set_forced_playouts(*opts["forced"])
    if "gumbel" in opts:
        e.set_gumbel(opts["gumbel"])
    if opts.get("mirror"):
        e.set_eval_mirror(True)


@pytest.fixture(autouse=True)
def options_off_afterwards(eng):
    yield
    set_options(eng, {})
    eng.set_option("selfplay_record_search", 0)


def played(e, noise=None, n_games=6):
    """A short hash-net self-play with the search record on: its first N tuples as positions, with the game id and the recorded prior of each."""
    set_options(e, {"noise": noise} if noise else {})
    e.set_option("selfplay_record_search", 1)
    got = e.selfplay(n_games=n_games, num_sims=SIMS, model_id=HASH, seed=SEED, first_game_id=FIRST, symmetries=False, want_boards=False)
    _, prior = e.selfplay_search()
    e.set_option("selfplay_record_search", 0)
    set_options(e, {})
    ids = np.repeat(FIRST + np.arange(n_games, dtype=np.uint64), got["game_len"].astype(np.int64))
    assert got["count"] == len(ids) >= N
    out = {"states": got["states"][:N].copy(), "game_ids": ids[:N].copy(), "prior": prior[:N].copy()}
    for a in out.values():
        a.setflags(write=False)
    return out


_played = {}


@pytest.fixture(scope="module")
def window(eng):
    if "plain" not in _played:
        _played["plain"] = played(eng)
    w = _played["plain"]
    stones = np.array([bin(int(a | b)).count("1") for a, b in w["states"]])
    assert (stones == 0).sum() >= 2 and stones.max() >= 15 and len(np.unique(w["game_ids"])) >= 2      # all plies, duplicates left in
    return w


def one_tree_rows(e, states, game_ids, model_id, sims, temp, seed=SEED, threads=1, reserve=None):
    """The definition: a one-tree batch, reset to each position and asked once.  Returns the rows and the summed stats of the n calls."""
    n = len(states)
    out = {"pi": np.zeros((n, 7), np.float32), "counts": np.zeros((n, 7), np.uint16), "q": np.zeros((n, 7), np.float32),
           "selected": np.zeros(n, np.int32)}
    tb = e.tree_create(1, reserve=reserve or tw.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=model_id, cpuct=1, num_threads=threads)
    e.reset_stats()
    try:
        for i in range(n):
            tb.reset(states[i:i + 1])
            out["pi"][i], out["counts"][i], out["q"][i] = (x[0] for x in tb.get_action_prob(states[i:i + 1], temp, seed=seed, first_game_id=int(game_ids[i])))
            out["selected"][i] = tb.selected()[0]
    finally:
        tb.close()
    out["stats"] = e.stats()
    return out


def reanalysed(e, w, model_id, sims=SIMS, temp=1.0, seed=SEED, threads=1, concurrent=CONCURRENT, **kw):
    e.reset_stats()
    kw.setdefault("states", w["states"])
    kw.setdefault("game_ids", w["game_ids"])
    got = e.reanalyse(sims, model_id, temp=temp, seed=seed, concurrent=concurrent, reserve=tw.default_reserve(sims), num_sim_threads=threads, **kw)
    got["stats"] = e.stats()
    return got


def same(a, b, keys):
    for k in keys:
        assert fg.same_rows(np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])), k


# ---- 1. rows equal the one-tree calls ------------------------------------------------------------------------------------------------------
ROWS = {
    "hash": dict(model=HASH),
    "hash_temp0": dict(model=HASH, temp=0.0),
    "conv": dict(model=CONV),
    "conv_temp0": dict(model=CONV, temp=0.0),
    "hash_dedup0": dict(model=HASH, options={"eval_dedup": 0}),
    "hash_dedup2": dict(model=HASH, options={"eval_dedup": 2}),
    "conv_dedup0": dict(model=CONV, options={"eval_dedup": 0}),
    "conv_dedup2": dict(model=CONV, options={"eval_dedup": 2}),
    "hash_per_sim": dict(model=HASH, options={"fused_search": 0}),
    "hash_fused": dict(model=HASH, options={"fused_search": 1}),
    "hash_threads5": dict(model=HASH, threads=5),
    "conv_threads5": dict(model=CONV, threads=5),
    "hash_noise": dict(model=HASH, noise=(0.25, 1.0)),
    "conv_noise": dict(model=CONV, noise=(0.25, 0.5)),
    "hash_forced_prune": dict(model=HASH, forced=(2.0, True)),
    "conv_forced_prune": dict(model=CONV, forced=(2.0, True)),
    "hash_gumbel4": dict(model=HASH, gumbel=4, sims=16),
    "hash_gumbel4_temp0": dict(model=HASH, gumbel=4, sims=16, temp=0.0),
    "conv_gumbel4": dict(model=CONV, gumbel=4, sims=16),
    "conv_mirror": dict(model=CONV, mirror=True),
    "conv_fp8": dict(model=CONV_FP8),
}
_refs = {}


def reference(e, w, name):
    """The one-tree rows of a parameter row under its own options (computed once, shared, left unchanged)."""
    if name not in _refs:
        row = ROWS[name]
        set_options(e, row)
        ref = one_tree_rows(e, w["states"], w["game_ids"], row["model"], row.get("sims", SIMS), row.get("temp", 1.0), threads=row.get("threads", 1))
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[name] = ref
    return _refs[name]


@pytest.mark.parametrize("name", list(ROWS))
def test_rows_equal_the_one_tree_calls(eng, window, name):
    row = ROWS[name]
    ref = reference(eng, window, name)
    set_options(eng, row)
    got = reanalysed(eng, window, row["model"], sims=row.get("sims", SIMS), temp=row.get("temp", 1.0), threads=row.get("threads", 1))
    same(got, ref, ("pi", "counts", "q", "selected"))
    sims = row.get("sims", SIMS)
    if "gumbel" in row:
        assert (got["selected"] >= 0).all() and (got["selected"] < 7).all()
    else:
        assert (got["selected"] == -1).all()
    st, rs = got["stats"], ref["stats"]
    assert st["moves"] == N == rs["moves"]
    for k in SUMMED:
        assert st[k] == rs[k], (k, st[k], rs[k])
    if "threads" not in row:                                       # (several in flight: a simulation may be abandoned)
        assert st["simulations"] == N * sims and (got["counts"].astype(np.int64).sum(axis=1) == sims).all()
    assert st["leaf_rows_executed"] <= rs["leaf_rows_executed"]


def test_bit_identical_switches_share_one_answer(eng, window):
    """eval_dedup and fused_search never change a result: their rows' references are the plain reference, and the classes differ."""
    for model, names in ((HASH, ("hash_dedup0", "hash_dedup2", "hash_per_sim", "hash_fused")), (CONV, ("conv_dedup0", "conv_dedup2"))):
        plain = reference(eng, window, "hash" if model == HASH else "conv")
        for n in names:
            same(reference(eng, window, n), plain, ("pi", "counts", "q"))
    assert not np.array_equal(reference(eng, window, "conv")["q"], reference(eng, window, "conv_fp8")["q"])
    assert not np.array_equal(reference(eng, window, "hash")["pi"], reference(eng, window, "hash_noise")["pi"])


# ---- 2. root_q and root_prior ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hash", "conv", "hash_threads5", "hash_forced_prune", "hash_gumbel4"])
def test_root_q_is_the_rule_of_az_target(eng, window, name):
    row = ROWS[name]
    set_options(eng, row)
    got = reanalysed(eng, window, row["model"], sims=row.get("sims", SIMS), threads=row.get("threads", 1))
    want = np.array([tt.root_value_py(c, q) for c, q in zip(got["counts"], got["q"])], np.float32)
    assert fg.same_rows(got["root_q"], want)
    assert np.all(np.abs(got["root_q"]) <= 1.0) and np.any(got["root_q"] != 0.0)


@pytest.mark.parametrize("noise", [None, (0.25, 1.0)])
def test_root_prior_is_what_selfplay_recorded(eng, window, noise):
    """With the self-play's own seed and game ids a fresh root stores the priors the playing tree stored: the net's answer for the state,
    and with root noise on the noise of (seed, game id, ply) mixed in."""
    key = "noise" if noise else "plain"
    if key not in _played:
        _played[key] = played(eng, noise)
    w = _played[key]
    set_options(eng, {"noise": noise} if noise else {})
    got = reanalysed(eng, w, HASH)
    assert fg.same_rows(got["root_prior"], w["prior"])
    valid = np.array([[not ((int(a) | int(b)) >> (c * 7 + 5)) & 1 for c in range(7)] for a, b in w["states"]])
    assert ((got["root_prior"] > 0) == valid).all()
    if noise:
        assert not np.array_equal(w["prior"][0], window["prior"][0])          # the empty board of the first game, with and without noise


# ---- 3. independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [HASH, CONV])
def test_concurrent_does_not_matter(eng, window, model):
    ref = reference(eng, window, "hash" if model == HASH else "conv")
    set_options(eng, {})
    first = None
    for c in (1, 7, 40, 70, 0):
        got = reanalysed(eng, window, model, concurrent=c)
        same(got, ref, ("pi", "counts", "q", "selected"))
        first = first or got
        same(got, first, OUT_KEYS)


def test_order_route_and_pointer_kind_do_not_matter(eng, window):
    from alphazero_rs_amd.coach import states_to_boards
    set_options(eng, {"noise": (0.25, 1.0)})                     # the game ids matter: they must travel with the positions
    base = reanalysed(eng, window, CONV)
    perm = np.random.default_rng(3).permutation(N)
    moved = reanalysed(eng, window, CONV, states=window["states"][perm], game_ids=window["game_ids"][perm])
    for k in OUT_KEYS:
        assert fg.same_rows(np.ascontiguousarray(moved[k]), np.ascontiguousarray(base[k][perm])), k
    wrong = reanalysed(eng, window, CONV, states=window["states"][perm])                  # ... and do: the ids left behind change the noise
    assert not np.array_equal(wrong["pi"], moved["pi"])
    by_boards = reanalysed(eng, window, CONV, states=None, boards=states_to_boards(window["states"]))
    same(by_boards, base, OUT_KEYS)
    # first_game_id + i when no ids are given
    run = reanalysed(eng, window, CONV, game_ids=None, first_game_id=77)
    ids = reanalysed(eng, window, CONV, game_ids=77 + np.arange(N, dtype=np.uint64))
    same(run, ids, OUT_KEYS)
    # device pointers in and out
    dev = torch.device("cuda", 0)
    d_states = torch.from_numpy(window["states"].view(np.int64).copy()).to(dev)
    d_ids = torch.from_numpy(window["game_ids"].view(np.int64).copy()).to(dev)
    out = {"pi": torch.zeros((N, 7), dtype=torch.float32, device=dev), "root_q": torch.zeros(N, dtype=torch.float32, device=dev),
           "root_prior": torch.zeros((N, 7), dtype=torch.float32, device=dev), "counts": torch.zeros((N, 7), dtype=torch.int16, device=dev),
           "q": torch.zeros((N, 7), dtype=torch.float32, device=dev), "selected": torch.zeros(N, dtype=torch.int32, device=dev)}
    reanalysed(eng, window, CONV, states=d_states, game_ids=d_ids, out=out)
    torch.cuda.synchronize()
    on_dev = {k: v.cpu().numpy() for k, v in out.items()}
    on_dev["counts"] = on_dev["counts"].view(np.uint16)
    same(on_dev, base, OUT_KEYS)
    # outputs that are not asked for are not needed
    only_pi = reanalysed(eng, window, CONV, out={"root_q": None, "root_prior": None, "counts": None, "q": None, "selected": None})
    assert fg.same_rows(only_pi["pi"], base["pi"])


def test_warm_persistent_cache_gives_the_same_bytes(engine_mod, window):
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    try:
        e.net_init_random(CONV, seed=3)
        cold = reanalysed(e, window, CONV)
        e.set_option("eval_cache_log2", 18)
        e.set_option("eval_cache_persist", 1)
        first = reanalysed(e, window, CONV)
        warm = reanalysed(e, window, CONV)
        same(first, cold, OUT_KEYS)
        same(warm, cold, OUT_KEYS)
        assert warm["stats"]["leaf_rows_requested"] == first["stats"]["leaf_rows_requested"] == cold["stats"]["leaf_rows_requested"]
        assert warm["stats"]["leaf_rows_executed"] < first["stats"]["leaf_rows_executed"]
        assert first["stats"]["leaf_rows_executed"] <= cold["stats"]["leaf_rows_executed"]
    finally:
        e.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def bit(c, r):
    return 1 << (c * 7 + r)


FULL_DRAW = [0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0, 2, 3, 2, 3, 2, 3, 3, 2, 3, 2, 3, 2, 4, 5, 4, 5, 4, 5, 5, 4, 5, 4, 5, 4, 6, 6, 6, 6, 6, 6]


def play(moves):
    mine, theirs = 0, 0
    for c in moves:
        mine, theirs = fg.c4_play(mine, theirs, c)
    return mine, theirs


BAD_POSITIONS = {
    "floating": ((0, bit(2, 1)), "a stone above an empty cell"),
    "counts": ((0, bit(0, 0) | bit(1, 0)), "stone counts"),
    "decided": (play([0, 0, 1, 1, 2, 2, 3]), "already decided or full"),
    "full": (play(FULL_DRAW), "already decided or full"),
    "outside": ((0, bit(4, 6)), "bits outside the 7x6 board"),
    "overlap": ((bit(3, 0), bit(3, 0)), "overlapping stones"),
}


def refused(engine_mod, call, status=AZ_ERR_BAD_ARGUMENT):
    with pytest.raises(engine_mod.AzError) as ei:
        call()
    assert ei.value.status == status, str(ei.value)
    return str(ei.value)


@pytest.mark.parametrize("name", list(BAD_POSITIONS))
@pytest.mark.parametrize("at", [0, 41, 69])
def test_bad_positions_are_refused_by_index(eng, engine_mod, window, name, at):
    (mine, theirs), text = BAD_POSITIONS[name]
    states = window["states"].copy()
    states[at] = (mine, theirs)
    if at == 41:
        states[60] = (bit(0, 3), 0)                                # a later offender is not the one that is named
    eng.reset_stats()
    pi = np.full((N, 7), 7.0, np.float32)
    msg = refused(engine_mod, lambda: eng.reanalyse(SIMS, HASH, states=states, concurrent=CONCURRENT, out={"pi": pi}))
    assert "az_reanalyse" in msg and ("position %d:" % at) in msg and text in msg, msg
    st = eng.stats()
    assert st["simulations"] == 0 and st["moves"] == 0 and (pi == 7.0).all()          # nothing searched, nothing written
    got = reanalysed(eng, window, HASH)                            # the engine is usable afterwards
    same(got, reference(eng, window, "hash"), ("pi", "counts", "q"))


def test_bad_features_are_refused_by_index(eng, engine_mod, window):
    from alphazero_rs_amd.coach import states_to_boards
    boards = states_to_boards(window["states"])
    boards[12, 0, 5, 3] = 0.5
    msg = refused(engine_mod, lambda: eng.reanalyse(SIMS, HASH, boards=boards))
    assert "position 12:" in msg and "a boards feature that is not 0 or 1" in msg
    boards = states_to_boards(window["states"])
    boards[33, 0, 0, 0] = 1.0                                       # a stone in the top row of an (at most half-full) column floats
    msg = refused(engine_mod, lambda: eng.reanalyse(SIMS, HASH, boards=boards))
    assert "position 33:" in msg


def test_bad_parameters_are_refused(eng, engine_mod, window):
    s = window["states"]
    eng.reset_stats()
    refused(engine_mod, lambda: eng.reanalyse(0, HASH, states=s))
    refused(engine_mod, lambda: eng.reanalyse(25, HASH, states=s, num_sim_threads=2))            # 25 % 2
    refused(engine_mod, lambda: eng.reanalyse(27, HASH, states=s, num_sim_threads=9))            # more than 8 threads
    refused(engine_mod, lambda: eng.reanalyse(25, HASH, states=s, reserve=7))
    refused(engine_mod, lambda: eng.reanalyse(25, HASH, states=s, concurrent=-1))
    refused(engine_mod, lambda: eng.reanalyse(25, CONV, states=s, concurrent=60, num_sim_threads=5))        # 300 rows > max_batch
    assert refused(engine_mod, lambda: eng.reanalyse(25, 99, states=s), status=6)                # AZ_ERR_NO_MODEL
    eng.set_gumbel(4)
    assert "gumbel_m" in refused(engine_mod, lambda: eng.reanalyse(25, HASH, states=s, num_sim_threads=5))
    eng.set_gumbel(0)
    eng.set_forced_playouts(2.0, True)
    assert "forced_playouts_k_e6" in refused(engine_mod, lambda: eng.reanalyse(25, HASH, states=s, num_sim_threads=5))
    eng.set_forced_playouts(0.0, False)
    # what the binding itself never passes: NULL pi, both position pointers NULL, n > 2^24 (refused before anything is read)
    p = engine_mod.az_reanalyse_params(0, 25, 1000, 1, HASH, 1, 1.0, 1000000, 0, 0)
    pi = np.zeros((N, 7), np.float32)
    raw = lambda n, st, pi_: eng._lib.az_reanalyse(eng._h, C.byref(p), n, st, None, None, pi_, None, None, None, None, None)
    sp, pp = s.ctypes.data_as(C.c_void_p), pi.ctypes.data_as(C.c_void_p)
    assert raw(N, sp, None) == AZ_ERR_BAD_ARGUMENT and b"pi is required" in eng._lib.az_last_error(eng._h)
    assert raw(N, None, pp) == AZ_ERR_BAD_ARGUMENT and b"states or boards" in eng._lib.az_last_error(eng._h)
    assert raw((1 << 24) + 1, sp, pp) == AZ_ERR_BAD_ARGUMENT and b"2^24" in eng._lib.az_last_error(eng._h)
    assert raw(-1, sp, pp) == AZ_ERR_BAD_ARGUMENT
    assert eng._lib.az_reanalyse(eng._h, None, N, sp, None, None, pp, None, None, None, None, None) == AZ_ERR_BAD_ARGUMENT
    assert eng.stats()["simulations"] == 0
    # n = 0 runs nothing and needs no array
    assert raw(0, None, None) == 0
    assert eng.reanalyse(25, HASH, states=np.zeros((0, 2), np.uint64))["pi"].shape == (0, 7)
    assert eng.stats()["moves"] == 0
    same(reanalysed(eng, window, HASH), reference(eng, window, "hash"), ("pi", "counts", "q"))


def test_the_second_game_is_refused(engine_mod, window):
    for e in fg.connect_three_engine(engine_mod):
        msg = refused(engine_mod, lambda: e.reanalyse(SIMS, HASH, states=window["states"]))
        assert "Connect Four" in msg


def test_a_full_tree_names_a_position(eng, engine_mod, window):
    msg = refused(engine_mod, lambda: eng.reanalyse(SIMS, HASH, states=window["states"], concurrent=CONCURRENT, reserve=8), status=AZ_ERR_CAPACITY)
    assert "az_reanalyse: position 0:" in msg, msg
    tb = eng.tree_create(1, reserve=8, num_sims=SIMS, max_depth=1000, model_id=HASH, cpuct=1)      # ... as the one-tree call runs full
    tb.reset(window["states"][:1])
    refused(engine_mod, lambda: tb.get_action_prob(window["states"][:1], 1.0), status=AZ_ERR_CAPACITY)
    tb.close()
    same(reanalysed(eng, window, HASH), reference(eng, window, "hash"), ("pi", "counts", "q"))


# ---- 5. session and purity ------------------------------------------------------------------------------------------------------------------
class Interrupting:
    """The engine as feature_gpu.check_session_in_chunks drives it, with a refused az_reanalyse in front of every chunk."""

    def __init__(self, e, engine_mod, states):
        self._e, self._mod, self._states, self.refusals = e, engine_mod, states, 0

    def __getattr__(self, name):
        return getattr(self._e, name)

    def selfplay_next(self, k):
        before = self._e.stats()
        msg = refused(self._mod, lambda: self._e.reanalyse(SIMS, HASH, states=self._states))
        assert "az_reanalyse" in msg and "self-play session is open" in msg, msg
        assert self._e.stats() == before
        self.refusals += 1
        return self._e.selfplay_next(k)


@pytest.mark.parametrize("driver", [0, 1])
def test_refused_inside_an_open_session(eng, engine_mod, window, driver):
    set_options(eng, {})
    one = fg.run_selfplay(eng, SIMS, SEED, options={"selfplay_async": driver})
    proxy = Interrupting(eng, engine_mod, window["states"])
    fg.check_session_in_chunks(proxy, one, ((0, 30), (30, 30), (60, 40)),
                               dict(n_games=fg.N_GAMES, num_sims=SIMS, model_id=HASH, seed=SEED, first_game_id=1000, concurrent=fg.SLOTS))
    assert proxy.refusals == 3
    same(reanalysed(eng, window, HASH), reference(eng, window, "hash"), ("pi", "counts", "q"))       # and accepted again behind the session


def test_other_entry_points_do_not_see_it(eng, window):
    set_options(eng, {})
    before = fg.other_entry_points(eng)
    reanalysed(eng, window, HASH)
    reanalysed(eng, window, CONV, threads=5)
    fg.assert_same_outputs(fg.other_entry_points(eng), before)


def test_the_tree_arena_is_reused(eng, window):
    set_options(eng, {})
    reanalysed(eng, window, CONV)
    allocs = eng.stats()["tree_arena_allocs"]
    for _ in range(3):
        got = reanalysed(eng, window, CONV)
        assert got["stats"]["tree_arena_allocs"] == allocs
    same(got, reference(eng, window, "conv"), ("pi", "counts", "q"))


# ---- 6. the two Coaches ---------------------------------------------------------------------------------------------------------------------
CH, COACH_SEED, COACH_SIMS = 128, 11, 16


def run_py_coach(engine_mod, d, iters, sims, q=0.0):
    from alphazero_rs_amd.coach import Coach
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=CH)
    try:
        e.net_init_random(0, 3)
        e.set_option("train_epochs", 1)
        coach = Coach.setup(e, d, 1000000, 0.55, 15, 3, 100000, 1, 64, 8, iters, 16, 25, 1, 1000, 1, log=lambda m: None)
        coach.reanalyse_sims = sims
        coach.value_target_q = q
        return coach.learn(seed=COACH_SEED)
    finally:
        e.close()


@pytest.fixture(scope="module")
def cpp_coach(engine_mod, tmp_path_factory):
    exe = os.path.join(tmp_path_factory.mktemp("coach_reanalyse"), "test_coach_reanalyse")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_reanalyse.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])

    def run(d, iters, sims, q=0.0):
        out = subprocess.run([exe, d, str(CH), str(COACH_SEED), str(iters), str(sims), repr(q)], check=True, stdout=subprocess.PIPE, text=True,
                             timeout=600).stdout
        return json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    return run


def read_examples(path):
    from alphazero_rs_amd.coach import load_examples
    return load_examples(path)


def test_coaches_agree_and_resume(engine_mod, cpp_coach, tmp_path):
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp", "resumed", "plain", "off")}
    rep = run_py_coach(engine_mod, dirs["py"], 2, COACH_SIMS)
    crep = cpp_coach(dirs["cpp"], 2, COACH_SIMS)
    assert len(rep) == len(crep) == 2
    for a, b in zip(rep, crep):
        for k in fg.REPORT_KEYS + ("reanalysed",):
            assert a[k] == b[k], k
        assert a["t_reanalyse"] >= 0.0
    assert rep[0]["reanalysed"] == 0 and rep[1]["reanalysed"] > 0                       # iteration 0 has no older window
    fg.compare_directories(dirs["py"], dirs["cpp"], required=("0.examples", "1.examples", "1.aznet"))
    # resume behind iteration 0: byte-identical to the uninterrupted run
    run_py_coach(engine_mod, dirs["resumed"], 1, COACH_SIMS)
    rep2 = run_py_coach(engine_mod, dirs["resumed"], 1, COACH_SIMS)
    assert rep2[0]["iteration"] == 1 and rep2[0]["reanalysed"] == rep[1]["reanalysed"]
    fg.compare_directories(dirs["py"], dirs["resumed"], required=("0.examples", "1.examples"))
    # with 0 the files are a plain run's: the field's default, and the field set to 0
    from alphazero_rs_amd.coach import Coach
    run_py_coach(engine_mod, dirs["off"], 2, 0)
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=CH)
    try:
        e.net_init_random(0, 3)
        e.set_option("train_epochs", 1)
        plain = Coach.setup(e, dirs["plain"], 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 2, 16, 25, 1, 1000, 1, log=lambda m: None).learn(seed=COACH_SEED)
    finally:
        e.close()
    assert "reanalysed" not in plain[0]
    fg.compare_directories(dirs["plain"], dirs["off"], required=("0.examples", "1.examples"))
    # with 16, iteration 0's file is the plain run's and iteration 1's differs from it in the older window's pi only
    with open(os.path.join(dirs["py"], "0.examples"), "rb") as x, open(os.path.join(dirs["plain"], "0.examples"), "rb") as y:
        assert x.read() == y.read()
    got, want = read_examples(os.path.join(dirs["py"], "1.examples")), read_examples(os.path.join(dirs["plain"], "1.examples"))
    assert len(got) == len(want) == 2
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][2], want[0][2])       # the older window: boards and z kept
    assert not np.array_equal(got[0][1], want[0][1])                                             # ... its pi re-searched
    assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))                            # the new window: the same model played it
    assert np.allclose(got[0][1].sum(axis=1), 1.0, atol=1e-5) and rep[1]["reanalysed"] == len(got[0][2])


def test_coaches_agree_with_a_blended_z(engine_mod, cpp_coach, tmp_path):
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp")}
    rep = run_py_coach(engine_mod, dirs["py"], 2, COACH_SIMS, q=0.5)
    crep = cpp_coach(dirs["cpp"], 2, COACH_SIMS, q=0.5)
    for a, b in zip(rep, crep):
        for k in fg.REPORT_KEYS + ("reanalysed",):
            assert a[k] == b[k], k
    fg.compare_directories(dirs["py"], dirs["cpp"], required=("0.examples", "1.examples"))
