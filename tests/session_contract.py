"""The call-interleaving contract of an open self-play session as a TABLE (include/az_engine.h, next to az_selfplay_begin; DESIGN.md
section 4.3b): one row per export of include/az_engine.h and one per az_set_option key of the shipped library, each with its class and a
callable that makes the call with small valid arguments.  TEST INFRASTRUCTURE ONLY, a plain module imported the way feature_gpu is.

tests/test_session_contract_cpu.py keeps the table closed-world (an export or a key that is missing, or listed twice, fails the suite
before anything runs on a GPU); tests/test_session_contract_gpu.py holds every row to its class under both self-play drivers.

Classes
  REFUSED    AZ_ERR_BAD_ARGUMENT on entry with a message that names the entry; nothing changes
  BY_MODEL   REFUSED when the call's destination is the session's model id, INERT for any other id; the callable takes the id
  INERT      accepted; the session's remaining chunks are bit for bit the undisturbed session's, and the call returns what it returns on
             an engine with no session open
  OWN        the session's own entries and the handle's lifecycle (az_selfplay_next / _end, az_create / az_destroy, az_last_error, and
             az_set_option, whose class is its key's): they are what the tests drive the session with, not calls beside it

A row: Row(name, cls, call, prep=None, conv=False, compare=True)
  call(ctx) / call(ctx, model_id)   makes the call; raises engine.AzError when the library refuses; returns the call's own output
  prep(ctx)                         runs BEFORE az_selfplay_begin (and on the engine without a session): models, trees, a training session
  conv                              the row touches a conv net: it also runs beside a conv-net session, and prep gets conv models
  compare                           False where the output is the session's own data (its last chunk's masks, its counters)
"""
import ctypes
import os

import numpy as np

REFUSED, BY_MODEL, INERT, OWN = "refused", "by_model", "inert", "own"
CLASSES = (REFUSED, BY_MODEL, INERT, OWN)
OWN_ENTRIES = ("az_create", "az_destroy", "az_last_error", "az_set_option", "az_selfplay_next", "az_selfplay_end")

HASH_SALT = 1234
HASH_ID, HASH_OTHER = 10, 11          # the hash nets every engine of the tests has
CONV_ID, CONV_OTHER = 0, 1            # the conv nets of a row with conv = True
SCRATCH_ID = 7                        # never initialised when a session begins: the destination of the BY_MODEL rows' inert half
CHANNELS, MAX_BATCH = 128, 256


class Row:
    def __init__(self, name, cls, call, prep=None, conv=False, compare=True):
        self.name, self.cls, self.call, self.prep, self.conv, self.compare = name, cls, call, prep, conv, compare

    def __repr__(self):
        return "Row(%s, %s)" % (self.name, self.cls)


class Ctx:
    """What a row's callables see: the engine, its module, the session's model id (sid), another id of the same kind (other), the conv
    model a conv row reads (cid: the session's own in a conv-net session) and whatever prep left behind."""

    def __init__(self, mod, e, conv_session, tmp):
        self.mod, self.e, self.tmp = mod, e, str(tmp)
        self.sid, self.other = (CONV_ID, CONV_OTHER) if conv_session else (HASH_ID, HASH_OTHER)
        self.cid = CONV_ID
        self.tree = self.shared = self.slot = None

    def path(self, name):
        return os.path.join(self.tmp, name)


def make_engine(mod, conv):
    """An engine of the tests' small shape: two hash nets, "eval_dedup" 2 (the cache and the free-running driver apply to them); with
    conv two conv nets of 128 channels as well."""
    e = mod.Engine(device=0, max_batch=MAX_BATCH, net_channels=CHANNELS)
    e.set_option("eval_dedup", 2)
    e.net_set_kind(HASH_ID, mod.NET_HASH, HASH_SALT)
    e.net_set_kind(HASH_OTHER, mod.NET_HASH, HASH_SALT)
    if conv:
        e.net_init_random(CONV_ID, seed=3)
        e.net_init_random(CONV_OTHER, seed=4)
    return e


# ---- small valid arguments -----------------------------------------------------------------------------------------------------------------
def _play(mine, theirs, a):
    mask = mine | theirs
    nb = (mask + (1 << (a * 7))) & (0x3F << (a * 7))
    return theirs, mine | nb


def _positions():
    out, s = [], (0, 0)
    for a in (3, 3, 2, 4, 0, 6, 1, 5):          # eight legal, unfinished positions of 0 .. 7 stones
        out.append(s)
        s = _play(s[0], s[1], a)
    return np.array(out, np.uint64)


STATES = _positions()
N = len(STATES)
PIS = np.full((N, 7), 1.0 / 7.0, np.float32)
PIS[:, 3] += np.float32(1.0) - PIS.sum(axis=1, dtype=np.float32)
ZS = np.array([1, -1, 1, -1, 0.5, -0.5, 1, -1], np.float32)
GAME_IDS = np.arange(N, dtype=np.uint64)


def _boards(mod):
    return np.stack([mod.c4_features(int(s[0]), int(s[1])) for s in STATES]).astype(np.float32)


def _reserve(sims):
    return 8 + 42 * (7 * sims + 8)


def _status(ctx, fn):
    """fn() or, when the library refuses for a reason that has nothing to do with a session, its status: both engines then agree."""
    try:
        return fn()
    except ctx.mod.AzError as ex:
        return ("status", ex.status)


# ---- preparations --------------------------------------------------------------------------------------------------------------------------
def prep_tree(ctx):
    ctx.tree = ctx.e.tree_create(2, reserve=_reserve(10), num_sims=10, max_depth=1000, model_id=HASH_OTHER, cpuct=1)
    ctx.tree.record_evals(16)
    ctx.tree.get_action_prob(np.zeros((2, 2), np.uint64), 1.0, seed=3, first_game_id=40)


def prep_shared(ctx):
    ctx.shared = ctx.e.tree_create(2, reserve=_reserve(10), num_sims=10, max_depth=1000, model_id=HASH_OTHER, cpuct=1)
    ctx.shared.share(0)
    ctx.slot = ctx.shared.slot_acquire()
    ctx.shared.slot_get_action_prob(ctx.slot, (0, 0), 1.0, seed=31, game_id=5)


def prep_arena(ctx):
    ctx.e.arena(4, 5, new_model_id=HASH_OTHER, old_model_id=HASH_ID, seed=4, record_evals=8)


def prep_train_options(ctx):
    for key, val in (("train_epochs", 1), ("train_batch", 4), ("train_dropout_e6", 0)):
        ctx.e.set_option(key, val)


def prep_train_open(ctx):
    prep_train_options(ctx)
    ctx.e.train_begin(CONV_OTHER)
    ctx.e.train_step(_boards(ctx.mod), PIS, ZS, mask_seed=1, apply=True)


def prep_train_ema(ctx):
    ctx.e.set_option("train_ema_decay_e9", 900000000)
    prep_train_open(ctx)


def prep_comm(ctx):
    ctx.e.comm_init(0, 1, ctx.e.comm_local_id(1))


def prep_saved(ctx):
    ctx.e.net_save(CONV_OTHER, ctx.path("other.aznet"))


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------
def call_train(ctx, mid):
    ctx.e.train(CONV_OTHER, mid, _boards(ctx.mod), PIS, ZS)
    return ctx.e.net_get_params(mid)


def call_train_end(ctx, mid):
    ctx.e.train_begin(CONV_OTHER)                 # INERT beside a session; a begin on an open training session restarts it
    ctx.e.train_step(_boards(ctx.mod), PIS, ZS, mask_seed=2, apply=True)
    ctx.e.train_end(mid)
    return ctx.e.net_get_params(mid)


def call_train_ema(ctx, mid):
    ctx.e.train_ema(mid)
    return ctx.e.net_get_params(mid)


def call_set_params(ctx, mid):
    ctx.e.net_set_params(mid, ctx.e.net_get_params(CONV_OTHER))
    return ctx.e.predict_states(STATES, mid)


def call_init_random(ctx, mid):
    ctx.e.net_init_random(mid, seed=9)
    return ctx.e.predict_states(STATES, mid)


def call_load(ctx, mid):
    ctx.e.net_load(mid, ctx.path("other.aznet"))
    return ctx.e.predict_states(STATES, mid)


def call_set_kind(ctx, mid):
    ctx.e.net_set_kind(mid, ctx.mod.NET_HASH, 77)
    return ctx.e.predict_states(STATES, mid)


def call_free(ctx, mid):
    if mid != ctx.sid:
        ctx.e.net_set_kind(mid, ctx.mod.NET_STUB, 0)        # something to free, on both visits
    ctx.e.net_free(mid)
    return "freed"


def call_tree_create(ctx):
    t = ctx.e.tree_create(3, reserve=_reserve(10), num_sims=10, max_depth=1000, model_id=ctx.sid, cpuct=1)
    n = t.node_counts()
    t.close()
    return n


def call_tree_reset(ctx):
    ctx.tree.reset(STATES[:2])
    return ctx.tree.node_counts()


def call_slot_acquire(ctx):
    s = ctx.shared.slot_acquire()
    ctx.shared.slot_release(s)
    return s


def call_comm_init(ctx):
    ctx.e.comm_destroy()
    ctx.e.comm_init(0, 1, ctx.e.comm_local_id(1))
    return ctx.e.allreduce_u64([1, 2, 3])


def call_set_validation(ctx):
    ctx.e.train_set_validation(PIS, ZS, states=STATES)
    ctx.e.train_set_validation()
    return "ok"


def call_save(ctx):
    ctx.e.net_save(ctx.cid, ctx.path("saved.aznet"))
    with open(ctx.path("saved.aznet"), "rb") as f:
        return np.frombuffer(f.read(), np.uint8)


def call_book(ctx):
    ctx.e.arena_set_opening_book(STATES[2:3])
    ctx.e.arena_set_opening_book(np.zeros((0, 2), np.uint64))
    return "ok"


def call_stats(ctx):
    return sorted(ctx.e.stats())


def call_reset_stats(ctx):
    ctx.e.reset_stats()
    return ctx.e.stats()["games"]


def call_full_plies(ctx):
    mask = np.zeros(64, np.uint64)               # one word per episode of the last chunk (at most 32 in the tests' sessions)
    st = ctx.e._lib.az_selfplay_get_full_plies(ctx.e._h, mask.ctypes.data_as(ctypes.c_void_p))
    return st, mask


def call_evaluate(ctx):
    r = ctx.e.evaluate(ctx.sid, PIS, ZS, states=STATES, per_tuple=True)
    return [r["sums"], r["ce"], r["se"], r["kl_rows"]]


EXPORTS = [
    # ---- lifecycle
    Row("az_create", OWN, None),
    Row("az_destroy", OWN, None),
    Row("az_last_error", OWN, None),
    Row("az_set_option", OWN, None),                      # by key: OPTIONS below
    Row("az_get_stats", INERT, call_stats, compare=False),
    Row("az_reset_stats", INERT, call_reset_stats, compare=False),
    # ---- models
    Row("az_net_set_kind", BY_MODEL, call_set_kind),
    Row("az_net_free", BY_MODEL, call_free),
    Row("az_net_set_class", REFUSED, lambda c: c.e.net_set_class(CONV_OTHER, c.mod.NET_CLASS_BF16), conv=True),
    Row("az_net_get_class", INERT, lambda c: c.e.net_class(c.cid), conv=True),
    Row("az_net_init_random", BY_MODEL, call_init_random, conv=True),
    Row("az_net_load", BY_MODEL, call_load, prep=prep_saved, conv=True),
    Row("az_net_save", INERT, call_save, conv=True),
    Row("az_net_param_count", INERT, lambda c: c.e.net_param_count()),
    Row("az_net_set_params", BY_MODEL, call_set_params, conv=True),
    Row("az_net_get_params", INERT, lambda c: c.e.net_get_params(c.cid), conv=True),
    Row("az_net_predict", INERT, lambda c: c.e.predict(_boards(c.mod), c.sid), conv=True),
    Row("az_net_predict_states", INERT, lambda c: c.e.predict_states(STATES, c.sid), conv=True),
    Row("az_net_evaluate", INERT, call_evaluate, conv=True),
    # ---- training
    Row("az_net_train", BY_MODEL, call_train, prep=prep_train_options, conv=True),
    Row("az_net_train_history", INERT, lambda c: c.e.train_history()),
    Row("az_net_train_begin", INERT, lambda c: c.e.train_begin(CONV_OTHER), conv=True),
    Row("az_net_train_step", INERT, lambda c: c.e.train_step(_boards(c.mod), PIS, ZS, mask_seed=5, apply=False)[0], prep=prep_train_open, conv=True),
    Row("az_net_train_end", BY_MODEL, call_train_end, prep=prep_train_options, conv=True),
    Row("az_net_train_ema", BY_MODEL, call_train_ema, prep=prep_train_ema, conv=True),
    Row("az_net_train_step_info", INERT, lambda c: c.e.train_step_info(), prep=prep_train_open, conv=True),
    Row("az_net_train_samples", REFUSED, lambda c: c.e.train_samples(CONV_OTHER, SCRATCH_ID, PIS, ZS, states=STATES)),
    Row("az_net_train_draw", REFUSED, lambda c: c.e.train_draw(N, 1, batch=64)),
    Row("az_net_train_set_validation", INERT, call_set_validation),
    Row("az_net_train_validation", INERT, lambda c: c.e.train_validation()),
    Row("az_samples_holdout", REFUSED, lambda c: c.e.samples_holdout(0.5, 1, PIS, ZS, states=STATES)),
    # ---- trees
    Row("az_tree_create", INERT, call_tree_create),
    Row("az_tree_destroy", INERT, call_tree_create),
    Row("az_tree_reset", INERT, call_tree_reset, prep=prep_tree),
    Row("az_tree_get_action_prob", REFUSED, lambda c: c.tree.get_action_prob(np.zeros((2, 2), np.uint64), 1.0), prep=prep_tree),
    Row("az_tree_record_evals", INERT, lambda c: c.tree.record_evals(4), prep=prep_tree),
    Row("az_tree_get_evals", INERT, lambda c: c.tree.get_evals(), prep=prep_tree),
    Row("az_tree_node_counts", INERT, lambda c: c.tree.node_counts(), prep=prep_tree),
    Row("az_tree_get_selected", INERT, lambda c: c.tree.selected(), prep=prep_tree),
    Row("az_tree_share", REFUSED, lambda c: c.tree.share(0), prep=prep_tree),
    Row("az_tree_slot_acquire", INERT, call_slot_acquire, prep=prep_shared),
    Row("az_tree_slot_release", INERT, call_slot_acquire, prep=prep_shared),
    Row("az_tree_slot_get_action_prob", REFUSED, lambda c: c.shared.slot_get_action_prob(c.slot, (0, 0), 1.0, seed=31, game_id=5), prep=prep_shared),
    Row("az_tree_slot_error", INERT, lambda c: c.shared.slot_error(c.slot), prep=prep_shared),
    Row("az_tree_share_stats", INERT, lambda c: c.shared.share_stats(), prep=prep_shared),
    Row("az_root_noise_eta", INERT, lambda c: c.e.root_noise_eta(STATES, GAME_IDS, seed=3)),
    Row("az_gumbel_values", INERT, lambda c: c.e.gumbel_values(STATES, GAME_IDS, seed=3)),
    # ---- self-play
    Row("az_selfplay", REFUSED, lambda c: c.e.selfplay(n_games=2, num_sims=5, model_id=c.other, seed=1)),
    Row("az_selfplay_begin", REFUSED, lambda c: c.e.selfplay_begin(2, 5, c.other, seed=1)),
    Row("az_selfplay_next", OWN, None),
    Row("az_selfplay_end", OWN, None),
    Row("az_selfplay_get_evals", INERT, lambda c: _status(c, lambda: c.e.selfplay_get_evals(2, 4)), compare=False),
    Row("az_selfplay_get_full_plies", INERT, call_full_plies, compare=False),
    Row("az_selfplay_get_search", INERT, lambda c: _status(c, lambda: c.e.selfplay_search()), compare=False),
    # ---- tuples, solver
    Row("az_samples_merge", REFUSED, lambda c: c.e.merge_samples(PIS, ZS, states=STATES)),
    Row("az_samples_blend_z", REFUSED, lambda c: c.e.blend_z(ZS, ZS, 0.5)),
    Row("az_samples_surprise", REFUSED, lambda c: c.e.surprise(PIS, ZS, PIS, 0.5, 1, states=STATES)),
    Row("az_solve", REFUSED, lambda c: c.e.solve(STATES, max_nodes=64)),
    Row("az_move_quality", REFUSED, lambda c: c.e.move_quality(np.array([4], np.int32), np.array([[3, 3, 2, 4] + [0] * 38], np.uint8), max_nodes=64)),
    # ---- arena
    Row("az_arena", REFUSED, lambda c: c.e.arena(4, 5, new_model_id=HASH_OTHER, old_model_id=HASH_ID, seed=4)),
    Row("az_arena_get_evals", INERT, lambda c: c.e.arena_get_evals(0, 4, 8), prep=prep_arena),
    Row("az_arena_get_moves", INERT, lambda c: c.e.arena_get_moves(4), prep=prep_arena),
    Row("az_arena_set_opening_book", INERT, call_book),
    Row("az_arena_get_openings", INERT, lambda c: c.e.arena_get_openings(4), prep=prep_arena),
    Row("az_tournament", REFUSED, lambda c: c.e.tournament([HASH_ID, HASH_OTHER], 2, 5, seed=1)),
    Row("az_rating_fit", INERT, lambda c: c.mod.rating_fit(np.array([[[0, 0, 0], [3, 1, 2]], [[1, 3, 2], [0, 0, 0]]], np.uint64))),
    # ---- communicator (an in-process world of one rank: the collectives' own code without a second engine)
    Row("az_comm_unique_id", INERT, lambda c: _status(c, lambda: len(c.e.comm_unique_id()))),
    Row("az_comm_local_id", INERT, lambda c: len(c.e.comm_local_id(1))),
    Row("az_comm_init", INERT, call_comm_init),
    Row("az_comm_destroy", INERT, lambda c: c.e.comm_destroy(), prep=prep_comm),
    Row("az_gather_samples", INERT, lambda c: c.e.gather_samples(STATES, PIS, ZS, dst=0, capacity=N), prep=prep_comm),
    Row("az_allreduce_u64", INERT, lambda c: c.e.allreduce_u64([5, 6, 7]), prep=prep_comm),
]


def _opt(key, cls, value, conv=False):
    return Row(key, cls, lambda c, key=key, value=value: c.e.set_option(key, value), conv=conv)


# value: a legal one that differs from the key's default, so that an accepted call changes something
OPTIONS = [
    # what a net computes, what a search returns, what the session captured at begin
    _opt("conv2_table", REFUSED, 0, conv=True),
    _opt("net_fp8", REFUSED, 1, conv=True),
    _opt("eval_mirror", REFUSED, 1, conv=True),
    _opt("eval_dedup", REFUSED, 1),
    _opt("eval_cache_log2", REFUSED, 12),
    _opt("eval_cache_persist", REFUSED, 1),
    _opt("eval_cache_max_stones", REFUSED, 10),
    _opt("selfplay_async", REFUSED, 1),
    _opt("selfplay_async_launches", REFUSED, 3),
    _opt("selfplay_async_iters", REFUSED, 8),
    _opt("root_noise_eps_e6", REFUSED, 250000),
    _opt("root_noise_alpha_e6", REFUSED, 300000),
    _opt("playout_cap_sims", REFUSED, 5),
    _opt("playout_cap_full_e6", REFUSED, 500000),
    _opt("forced_playouts_k_e6", REFUSED, 2000000),
    _opt("policy_prune", REFUSED, 1),
    _opt("gumbel_m", REFUSED, 4),
    _opt("gumbel_c_visit_e6", REFUSED, 1000000),
    _opt("gumbel_c_scale_e6", REFUSED, 2000000),
    _opt("selfplay_record_search", REFUSED, 1),
    # keys the shipped library refuses with or without a session (they print the diagnostic library's clock stamps)
    _opt("print_clock_stamps", REFUSED, 0),
    _opt("print_seg_stamps", REFUSED, 0),
    _opt("print_tree_stamps", REFUSED, 0),
    # the bit-identical kernel and schedule switches
    _opt("conv3_small", INERT, 0, conv=True),
    _opt("conv3_tail", INERT, 0, conv=True),
    _opt("conv3_planes", INERT, 0, conv=True),
    _opt("conv3_wreg", INERT, 0, conv=True),
    _opt("ring_packed", INERT, 0, conv=True),
    _opt("narrow_rows", INERT, 0, conv=True),
    _opt("tree_block4", INERT, 0),
    _opt("search_graph", INERT, 0, conv=True),
    _opt("search_graph_rows", INERT, 4),
    _opt("fused_search", INERT, 0),
    _opt("dedup_stats", INERT, 0),
    _opt("profile", INERT, 1),
    _opt("profile_every", INERT, 3),
    # only az_arena reads it, and az_arena is refused
    _opt("arena_opening_plies", INERT, 4),
    # the trainer's keys: no self-play path reads them
    _opt("train_epochs", INERT, 2),
    _opt("train_batch", INERT, 32),
    _opt("train_seed", INERT, 5),
    _opt("train_graph", INERT, 0),
    _opt("train_gemm3_ring", INERT, 0),
    _opt("train_fwd_x3", INERT, 0),
    _opt("train_wgrad_tr", INERT, 0),
    _opt("train_implicit", INERT, 0),
    _opt("train_fork", INERT, 1),
    _opt("train_gemm", INERT, 0),
    _opt("train_fwd_dma", INERT, 0),
    _opt("train_lr_e9", INERT, 2000000),
    _opt("train_dropout_e6", INERT, 100000),
    _opt("train_keep_best", INERT, 1),
    _opt("train_patience", INERT, 2),
    _opt("train_weight_decay_e9", INERT, 1000000),
    _opt("train_clip_norm_e6", INERT, 1000000),
    _opt("train_lr_warmup_steps", INERT, 3),
    _opt("train_lr_decay", INERT, 1),
    _opt("train_lr_floor_e6", INERT, 100000),
    _opt("train_lr_total_steps", INERT, 10),
    _opt("train_ema_decay_e9", INERT, 900000000),
    # the superseded kernel generations live in the diagnostic library; the shipped one accepts their default value and nothing else
    _opt("gemm_variant", INERT, 5),
    _opt("fc_ring", INERT, 1),
    _opt("ring_tile", INERT, 30000),
    _opt("conv3_ring", INERT, 0),
    _opt("conv2_pipe", INERT, 1),
    _opt("conv3_pipe", INERT, 1),
    _opt("conv1_table", INERT, 1),
    _opt("conv4_big", INERT, 0),
    _opt("tree_stamps", INERT, 0),
]

ROWS = EXPORTS + OPTIONS
