"""ctypes mirror of the C ABI in include/az_engine.h.

Names follow the reference's surface: `Engine.net_*` is the `NNet` trait
(src/nnet.rs:35-45), `TreeBatch` is n x `AsyncMcts` (src/async_mcts.rs:14-115),
`Engine.selfplay` is `Coach::execute_episode` x many (src/coach.rs:104-157) and
`Engine.arena` is `arena::play_games` (src/arena.rs:62-99).

The HIP library is mandatory: if it has not been built this module raises at
import -- there is no CPU path.
"""
import ctypes as C
import os
import weakref

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AZ_ENGINE_LIB") or os.path.join(_PKG, "libaz_engine.so")      # AZ_ENGINE_LIB: A/B of two builds (tools/)
# The diagnostic twin (built with -DAZ_DIAG): the same ABI plus the superseded kernel generations, forced tiles and clock-stamp builds
# behind az_set_option (none of them computes a wrong answer).  tools/ and the kernel-family bit-identity tests use it (Engine(diag=True)); nothing else.
DIAG_LIB_PATH = os.path.join(_PKG, "libaz_engine_diag.so")

ACTIONS = 7
FEATURES = 84
MAX_PLIES = 42

AZ_OK = 0
STATUS_NAMES = {
    0: "AZ_OK", 1: "AZ_ERR_BAD_ARGUMENT", 2: "AZ_ERR_CAPACITY", 3: "AZ_ERR_HIP", 4: "AZ_ERR_INVALID_MOVE",
    5: "AZ_ERR_TERMINAL_ROOT", 6: "AZ_ERR_NO_MODEL", 7: "AZ_ERR_IO", 8: "AZ_ERR_UNSUPPORTED",
}
NET_STUB, NET_HASH, NET_CONV = 0, 1, 2
GAME_CONNECT_FOUR, GAME_CONNECT_THREE = 0, 1
NET_CLASS_ENGINE, NET_CLASS_BF16, NET_CLASS_FP8 = -1, 0, 1      # az_net_class
SOLVE_ILLEGAL, SOLVE_UNKNOWN = -128, 127                         # AZ_SOLVE_ILLEGAL / AZ_SOLVE_UNKNOWN
MQ_SKIPPED, MQ_KEPT, MQ_WIN_TO_DRAW, MQ_WIN_TO_LOSS, MQ_DRAW_TO_LOSS, MQ_UNKNOWN = range(6)      # AZ_MQ_*: classes of az_move_quality
MQ_NAMES = ("skipped", "kept", "win_to_draw", "win_to_loss", "draw_to_loss", "unknown")
MERGE_CANONICAL = 1                                              # AZ_MERGE_CANONICAL, flags bit 0 of az_samples_merge
TRAIN_EPOCH_BY_WEIGHT, TRAIN_MIRROR = 1, 2                       # AZ_TRAIN_*: flags of az_net_train_samples / az_net_train_draw


class AzError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class az_config(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_batch", C.c_int32), ("net_channels", C.c_int32), ("profile", C.c_int32),
                ("game", C.c_int32)]


class az_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("games", "moves", "simulations", "expansions", "leaf_evals", "link_hits",
                                          "terminal_hits", "depth_sum", "samples", "net_launches")] + \
               [(n, C.c_double) for n in ("net_conv2_ms", "net_conv2_flops", "net_total_ms", "net_total_flops",
                                          "tree_ms", "tree_bytes", "device_ms")] + \
               [(n, C.c_uint64) for n in ("leaf_rows_requested", "leaf_rows_executed", "eval_cache_hits", "eval_batch_dups",
                                          "eval_cache_inserts")] + \
               [(n, C.c_double) for n in ("net_conv3_ms", "net_conv3_flops", "net_conv2_bytes")] + \
               [(n, C.c_uint64) for n in ("tree_launches", "tree_launches_timed", "tree_arena_allocs")] + \
               [(n, C.c_double) for n in ("net_conv4_ms", "net_conv4_flops", "net_fc_ms", "net_fc_flops", "net_rows_timed")] + \
               [("abandoned_sims", C.c_uint64), ("net_conv3_image_rows", C.c_uint64), ("net_conv3_image_launches", C.c_uint64)]


class az_selfplay_params(C.Structure):
    _fields_ = [("n_games", C.c_int32), ("concurrent", C.c_int32), ("num_sims", C.c_int32),
                ("temp_threshold", C.c_int32), ("max_depth", C.c_int32), ("cpuct", C.c_int32),
                ("model_id", C.c_int32), ("symmetries", C.c_int32), ("reserve", C.c_uint64), ("seed", C.c_uint64),
                ("first_game_id", C.c_uint64), ("record_evals", C.c_int32), ("num_sim_threads", C.c_int32)]


class az_samples(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("count", C.c_int64), ("states", C.c_void_p), ("boards", C.c_void_p),
                ("pis", C.c_void_p), ("zs", C.c_void_p), ("game_len", C.c_void_p), ("moves", C.c_void_p)]


class az_arena_params(C.Structure):
    _fields_ = [("num_games", C.c_int32), ("num_sims", C.c_int32), ("max_depth", C.c_int32), ("cpuct", C.c_int32),
                ("new_model_id", C.c_int32), ("old_model_id", C.c_int32), ("reserve", C.c_uint64), ("seed", C.c_uint64),
                ("first_game", C.c_int32), ("total_games", C.c_int32), ("record_evals", C.c_int32), ("num_sim_threads", C.c_int32),
                ("use_start_board", C.c_int32), ("allreduce_wld", C.c_int32), ("start_board", C.c_uint64 * 2)]


# every symbol include/az_engine.h declares (tests check the library exports all of them)
EXPORTS = [
    "az_create", "az_destroy", "az_last_error", "az_set_option", "az_get_stats", "az_reset_stats", "az_net_set_kind", "az_net_free",
    "az_net_set_class", "az_net_get_class",
    "az_net_init_random", "az_net_load", "az_net_save", "az_net_param_count", "az_net_set_params",
    "az_net_get_params", "az_net_predict", "az_net_predict_states", "az_net_train", "az_net_train_history",
    "az_net_train_begin", "az_net_train_step", "az_net_train_end", "az_net_train_ema", "az_net_train_step_info",
    "az_net_train_samples", "az_net_train_draw", "az_net_evaluate", "az_samples_holdout", "az_net_train_set_validation",
    "az_net_train_validation", "az_tree_create",
    "az_tree_destroy", "az_tree_reset", "az_tree_get_action_prob", "az_tree_record_evals", "az_tree_get_evals",
    "az_tree_node_counts", "az_tree_share", "az_tree_slot_acquire", "az_tree_slot_release", "az_tree_slot_get_action_prob",
    "az_tree_slot_error", "az_tree_share_stats", "az_root_noise_eta", "az_tree_get_selected", "az_gumbel_values", "az_selfplay", "az_selfplay_begin", "az_selfplay_next", "az_selfplay_end", "az_selfplay_get_evals", "az_selfplay_get_full_plies", "az_selfplay_get_search", "az_samples_merge", "az_samples_blend_z", "az_samples_surprise", "az_solve", "az_move_quality", "az_arena", "az_arena_get_evals", "az_arena_get_moves",
    "az_arena_set_opening_book", "az_arena_get_openings", "az_tournament", "az_rating_fit",
    "az_comm_unique_id", "az_comm_local_id", "az_comm_init", "az_comm_destroy", "az_gather_samples", "az_allreduce_u64",
]
COMM_ID_BYTES = 128


class az_reanalyse_params(C.Structure):
    _fields_ = [("concurrent", C.c_int32), ("num_sims", C.c_int32), ("max_depth", C.c_int32), ("cpuct", C.c_int32), ("model_id", C.c_int32),
                ("num_sim_threads", C.c_int32), ("temp", C.c_float), ("reserve", C.c_uint64), ("seed", C.c_uint64), ("first_game_id", C.c_uint64)]


# the symbols of the extension headers (include/az_reanalyse.h): exported by the same library, declared outside include/az_engine.h
EXT_EXPORTS = ["az_reanalyse"]
REANALYSE_ID_BASE = 1 << 62
# the symbols of include/az_search_stop.h (the decided-move stop): a list of their own, bound with the same skip
SEARCH_STOP_EXPORTS = ["az_search_stop_set", "az_search_stop_get", "az_search_stop_stats"]


def reanalyse_first_game_id(iteration, history_index):
    """csrc/az_reanalyse.h: the first game id of the Coach's re-search of history entry `history_index` in iteration `iteration`."""
    return (REANALYSE_ID_BASE + (int(iteration) << 40) + (int(history_index) << 32)) & (2 ** 64 - 1)


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP engine has not been built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc cross-compiles for gfx950 without a GPU). There is no CPU fallback.")
    lib = C.CDLL(path)
    vp, i32, u64, i64, f32 = C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_float
    sigs = {
        "az_create": (i32, [C.POINTER(az_config), C.POINTER(vp)]),
        "az_destroy": (None, [vp]),
        "az_last_error": (C.c_char_p, [vp]),
        "az_set_option": (i32, [vp, C.c_char_p, i64]),
        "az_get_stats": (i32, [vp, C.POINTER(az_stats)]),
        "az_reset_stats": (i32, [vp]),
        "az_net_set_kind": (i32, [vp, i32, i32, u64]),
        "az_net_init_random": (i32, [vp, i32, u64]),
        "az_net_free": (i32, [vp, i32]),
        "az_net_set_class": (i32, [vp, i32, i32]),
        "az_net_get_class": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32)]),
        "az_net_load": (i32, [vp, i32, C.c_char_p]),
        "az_net_save": (i32, [vp, i32, C.c_char_p]),
        "az_net_param_count": (i64, [vp]),
        "az_net_set_params": (i32, [vp, i32, vp, i64]),
        "az_net_get_params": (i32, [vp, i32, vp, i64]),
        "az_net_predict": (i32, [vp, i32, vp, i32, vp, vp]),
        "az_net_predict_states": (i32, [vp, i32, vp, i32, vp, vp]),
        "az_net_train": (i32, [vp, i32, i32, vp, vp, vp, i64]),
        "az_net_train_history": (i32, [vp, vp, i32]),
        "az_net_train_begin": (i32, [vp, i32]),
        "az_net_train_step": (i32, [vp, vp, vp, vp, i32, u64, i32, vp, vp]),
        "az_net_train_end": (i32, [vp, i32]),
        "az_net_train_ema": (i32, [vp, i32]),
        "az_net_train_step_info": (i32, [vp, vp]),
        "az_net_train_samples": (i32, [vp, i32, i32, C.POINTER(az_samples), vp, i32]),
        "az_net_train_draw": (i32, [vp, i64, vp, i32, u64, i64, vp, vp]),
        "az_net_evaluate": (i32, [vp, i32, C.POINTER(az_samples), vp, vp, vp, vp, vp, vp]),
        "az_samples_holdout": (i32, [vp, C.POINTER(az_samples), i64, u64, vp]),
        "az_net_train_set_validation": (i32, [vp, C.POINTER(az_samples), vp]),
        "az_net_train_validation": (i32, [vp, vp, i32, C.POINTER(i32)]),
        "az_tree_create": (i32, [vp, i32, u64, i32, i32, i32, i32, i32, C.POINTER(vp)]),
        "az_tree_destroy": (None, [vp]),
        "az_tree_reset": (i32, [vp, vp]),
        "az_tree_get_action_prob": (i32, [vp, vp, f32, u64, u64, vp, vp, vp]),
        "az_tree_record_evals": (i32, [vp, i32]),
        "az_tree_get_evals": (i32, [vp, vp, vp, vp, vp]),
        "az_tree_node_counts": (i32, [vp, vp]),
        "az_tree_share": (i32, [vp, i32]),
        "az_tree_slot_acquire": (i32, [vp, C.POINTER(i32)]),
        "az_tree_slot_release": (i32, [vp, i32]),
        "az_tree_slot_get_action_prob": (i32, [vp, i32, vp, f32, u64, u64, vp, vp, vp]),
        "az_tree_slot_error": (C.c_char_p, [vp, i32]),
        "az_tree_share_stats": (i32, [vp, vp]),
        "az_root_noise_eta": (i32, [vp, i32, u64, vp, vp, vp]),
        "az_tree_get_selected": (i32, [vp, vp]),
        "az_gumbel_values": (i32, [vp, i32, u64, vp, vp, i32, vp]),
        "az_selfplay": (i32, [vp, C.POINTER(az_selfplay_params), C.POINTER(az_samples)]),
        "az_selfplay_begin": (i32, [vp, C.POINTER(az_selfplay_params)]),
        "az_selfplay_next": (i32, [vp, C.c_int32, C.POINTER(az_samples)]),
        "az_selfplay_end": (i32, [vp]),
        "az_selfplay_get_evals": (i32, [vp, vp, vp, vp, vp]),
        "az_selfplay_get_full_plies": (i32, [vp, vp]),
        "az_samples_merge": (i32, [vp, C.POINTER(az_samples), i32, C.POINTER(az_samples), vp]),
        "az_selfplay_get_search": (i32, [vp, vp, vp]),
        "az_samples_blend_z": (i32, [vp, i64, vp, vp, i64, vp]),
        "az_samples_surprise": (i32, [vp, C.POINTER(az_samples), vp, i64, u64, C.POINTER(az_samples), vp, vp]),
        "az_solve": (i32, [vp, vp, i32, C.c_uint32, i32, i32, i32, vp, vp, vp]),
        "az_move_quality": (i32, [vp, vp, vp, vp, i32, C.c_uint32, i32, i32, i32, vp, vp]),
        "az_arena": (i32, [vp, C.POINTER(az_arena_params), vp, vp]),
        "az_arena_get_evals": (i32, [vp, i32, vp, vp, vp, vp]),
        "az_arena_get_moves": (i32, [vp, vp, vp]),
        "az_arena_set_opening_book": (i32, [vp, vp, i32]),
        "az_arena_get_openings": (i32, [vp, vp, vp, vp]),
        "az_tournament": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, u64, u64, vp, vp]),
        "az_rating_fit": (i32, [vp, i32, C.c_double, vp, vp, vp]),
        "az_comm_unique_id": (i32, [vp, vp]),
        "az_comm_local_id": (i32, [vp, i32, vp]),
        "az_comm_init": (i32, [vp, i32, i32, vp]),
        "az_comm_destroy": (i32, [vp]),
        "az_gather_samples": (i32, [vp, C.POINTER(az_samples), i32, C.POINTER(az_samples), vp]),
        "az_allreduce_u64": (i32, [vp, vp, i32]),
        # include/az_reanalyse.h (EXT_EXPORTS)
        "az_reanalyse": (i32, [vp, C.POINTER(az_reanalyse_params), i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        # include/az_search_stop.h (SEARCH_STOP_EXPORTS)
        "az_search_stop_set": (i32, [vp, i32]),
        "az_search_stop_get": (i32, [vp, C.POINTER(i32)]),
        "az_search_stop_stats": (i32, [vp, vp, i32]),
    }
    for name, (res, args) in sigs.items():
        if name in EXT_EXPORTS + SEARCH_STOP_EXPORTS and not hasattr(lib, name):      # an older build loaded through AZ_ENGINE_LIB (A/B runs): the entry's own method raises
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = load_library()
_lib_diag = None


def diag_library():
    global _lib_diag
    if _lib_diag is None:
        _lib_diag = load_library(DIAG_LIB_PATH)
    return _lib_diag


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _as_ptr(x):
    """numpy array -> host pointer; torch tensor -> its data_ptr() (device or host); int passes through."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


class Engine:
    """az_engine handle.  One per process per GPU (one HIP stream)."""

    def __init__(self, device=0, max_batch=8192, net_channels=512, profile=False, game=0, diag=False):
        cfg = az_config(device, max_batch, net_channels, 1 if profile else 0, game)
        h = C.c_void_p()
        self._lib = diag_library() if diag else _lib
        st = self._lib.az_create(C.byref(cfg), C.byref(h))
        if st != AZ_OK:
            raise AzError(st, "az_create failed (no usable HIP device?)")
        self._h = h
        self.net_channels = net_channels
        self._trees = weakref.WeakSet()

    def close(self):
        if self._h:
            for t in list(self._trees):   # a tree must not outlive its engine (it borrows the stream)
                t.close()
            self._lib.az_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != AZ_OK:
            raise AzError(st, self._lib.az_last_error(self._h).decode())

    # ---- NNet ----
    def net_set_kind(self, model_id, kind, salt=0):
        self._check(self._lib.az_net_set_kind(self._h, model_id, kind, salt))

    def net_free(self, model_id):
        """Drop a model id (weights + conv1 table); the per-stream activation workspace stays."""
        self._check(self._lib.az_net_free(self._h, model_id))

    def net_set_class(self, model_id, net_class):
        """az_net_set_class: pin ONE conv model to NET_CLASS_BF16 / NET_CLASS_FP8, or hand it back to the engine's "net_fp8" option
        (NET_CLASS_ENGINE, the default).  State of the id: it survives weight uploads, net_free drops it."""
        self._check(self._lib.az_net_set_class(self._h, model_id, int(net_class)))

    def net_class(self, model_id):
        """az_net_get_class -> (stored az_net_class, effective: 0 bf16 / 1 fp8)."""
        stored, effective = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.az_net_get_class(self._h, model_id, C.byref(stored), C.byref(effective)))
        return stored.value, effective.value

    def net_init_random(self, model_id, seed):
        self._check(self._lib.az_net_init_random(self._h, model_id, seed))

    def net_param_count(self):
        return int(self._lib.az_net_param_count(self._h))

    def net_set_params(self, model_id, params):
        p = np.ascontiguousarray(params, dtype=np.float32)
        self._check(self._lib.az_net_set_params(self._h, model_id, _ptr(p), p.size))

    def net_get_params(self, model_id):
        p = np.empty(self.net_param_count(), np.float32)
        self._check(self._lib.az_net_get_params(self._h, model_id, _ptr(p), p.size))
        return p

    def net_save(self, model_id, path):
        self._check(self._lib.az_net_save(self._h, model_id, os.fsencode(path)))

    def net_load(self, model_id, path):
        self._check(self._lib.az_net_load(self._h, model_id, os.fsencode(path)))

    def predict(self, boards, model_id):
        """NNet::predict: boards [B,2,6,7] f32 -> (pi [B,7], v [B])."""
        b = np.ascontiguousarray(boards, dtype=np.float32).reshape(-1, FEATURES)
        pi = np.empty((b.shape[0], ACTIONS), np.float32)
        v = np.empty(b.shape[0], np.float32)
        self._check(self._lib.az_net_predict(self._h, model_id, _ptr(b), b.shape[0], _ptr(pi), _ptr(v)))
        return pi, v

    def predict_states(self, states, model_id):
        s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 2)
        pi = np.empty((s.shape[0], ACTIONS), np.float32)
        v = np.empty(s.shape[0], np.float32)
        self._check(self._lib.az_net_predict_states(self._h, model_id, _ptr(s), s.shape[0], _ptr(pi), _ptr(v)))
        return pi, v

    def train(self, prev_id, model_id, boards, pis, vs):
        b = np.ascontiguousarray(boards, dtype=np.float32)
        p = np.ascontiguousarray(pis, dtype=np.float32)
        v = np.ascontiguousarray(vs, dtype=np.float32)
        self._check(self._lib.az_net_train(self._h, prev_id, model_id, _ptr(b), _ptr(p), _ptr(v), v.size))
        return self.train_history()

    @staticmethod
    def _train_flags(epoch_by_weight, mirror):
        return (TRAIN_EPOCH_BY_WEIGHT if epoch_by_weight else 0) | (TRAIN_MIRROR if mirror else 0)

    def train_samples(self, prev_id, model_id, pis, zs, *, states=None, boards=None, weights=None, epoch_by_weight=False, mirror=False):
        """az_net_train_samples: NNet::train on n tuples whose batch rows are drawn in proportion to `weights` (u32 [n], None = all
        ones: az_net_train's draw), mirrored at random with `mirror` (include/az_engine.h).  The position comes from `states` [n,2]
        -- the planes are then built per batch on the device -- or from `boards` [n,2,6,7] when states is None.  Inputs may be numpy
        arrays or torch tensors (host or device).  epoch_by_weight: an epoch has sum(weights) / batch steps, not n / batch."""
        if (states is None) == (boards is None):
            raise ValueError("train_samples takes states or boards, not both")
        n = int(len(zs))
        if not hasattr(pis, "data_ptr"):
            pis = np.ascontiguousarray(pis, dtype=np.float32).reshape(n, ACTIONS)
        if not hasattr(zs, "data_ptr"):
            zs = np.ascontiguousarray(zs, dtype=np.float32).reshape(n)
        if states is not None and not hasattr(states, "data_ptr"):
            states = np.ascontiguousarray(states, dtype=np.uint64).reshape(n, 2)
        if boards is not None and not hasattr(boards, "data_ptr"):
            boards = np.ascontiguousarray(boards, dtype=np.float32).reshape(n, 2, 6, 7)
        if weights is not None and not hasattr(weights, "data_ptr"):
            weights = np.ascontiguousarray(weights, dtype=np.uint32).reshape(n)
        src = az_samples(n, n, _as_ptr(states), _as_ptr(boards), _as_ptr(pis), _as_ptr(zs), None, None)
        self._check(self._lib.az_net_train_samples(self._h, prev_id, model_id, C.byref(src), _as_ptr(weights),
                                                   self._train_flags(epoch_by_weight, mirror)))
        return self.train_history()

    def train_draw(self, n, steps, *, weights=None, t0=0, batch, epoch_by_weight=False, mirror=False, out=None):
        """az_net_train_draw: the tuples (and mirror bits) of the `steps` batches of global steps t0 .. t0 + steps that train_samples
        would draw from n tuples with these weights, at the engine's current "train_seed" and "train_batch" -- `batch` must name
        that value (it sizes the outputs).  Runs the device prefix sum and the draw kernel alone.  Returns (idx [steps*batch] int64,
        mirror [steps*batch] uint8); out = (idx, mirror) writes into the caller's arrays or tensors (host or device) instead."""
        if weights is not None and not hasattr(weights, "data_ptr"):
            weights = np.ascontiguousarray(weights, dtype=np.uint32).reshape(int(n))
        rows = int(steps) * int(batch)
        idx, mir = out if out is not None else (np.full(max(rows, 0), -1, np.int64), np.full(max(rows, 0), 255, np.uint8))
        self._check(self._lib.az_net_train_draw(self._h, int(n), _as_ptr(weights), self._train_flags(epoch_by_weight, mirror), int(t0),
                                                int(steps), _as_ptr(idx), _as_ptr(mir)))
        return idx, mir

    def train_history(self):
        """[(loss_pi, loss_v)] per epoch of the last train()."""
        n = self._lib.az_net_train_history(self._h, None, 0)
        out = np.zeros((n, 2), np.float32)
        self._lib.az_net_train_history(self._h, _ptr(out), n)
        return [tuple(float(x) for x in r) for r in out]

    @staticmethod
    def _tuples(pis, zs, states, boards, weights):
        """(az_samples, weights, n) of a window given as numpy arrays or torch tensors (host or device); the arrays are returned so
        that they outlive the call."""
        if (states is None) == (boards is None):
            raise ValueError("states or boards, not both")
        n = int(len(zs))
        if not hasattr(pis, "data_ptr"):
            pis = np.ascontiguousarray(pis, dtype=np.float32).reshape(n, ACTIONS)
        if not hasattr(zs, "data_ptr"):
            zs = np.ascontiguousarray(zs, dtype=np.float32).reshape(n)
        if states is not None and not hasattr(states, "data_ptr"):
            states = np.ascontiguousarray(states, dtype=np.uint64).reshape(n, 2)
        if boards is not None and not hasattr(boards, "data_ptr"):
            boards = np.ascontiguousarray(boards, dtype=np.float32).reshape(n, 2, 6, 7)
        if weights is not None and not hasattr(weights, "data_ptr"):
            weights = np.ascontiguousarray(weights, dtype=np.uint32).reshape(n)
        return az_samples(n, n, _as_ptr(states), _as_ptr(boards), _as_ptr(pis), _as_ptr(zs), None, None), (pis, zs, states, boards, weights), n

    def evaluate(self, model_id, pis, zs, *, states=None, boards=None, weights=None, per_tuple=False, out=None):
        """az_net_evaluate: the held-out loss of model_id as self-play runs it (its effective class, "eval_mirror", any model kind) over
        the window (states [n,2] or boards [n,2,6,7], pis, zs; weights u32 [n], None = all ones), scored on the device in one call.
        Returns a dict: n, weight_sum, loss_pi, loss_v, kl, top1 (doubles from the integer sums) and sums = (S_ce, S_kl, S_se, S_hit, W).
        per_tuple adds the f32 arrays ce, se, kl [n]; out = (ce, se, kl) writes them into the caller's arrays or tensors instead."""
        src, keep, n = self._tuples(pis, zs, states, boards, weights)
        score = np.zeros(6, np.float64)
        sums = np.zeros(5, np.uint64)
        arrs = out if out is not None else (tuple(np.full(n, np.nan, np.float32) for _ in range(3)) if per_tuple else (None, None, None))
        self._check(self._lib.az_net_evaluate(self._h, model_id, C.byref(src), _as_ptr(keep[4]), _ptr(score), _ptr(sums),
                                              _as_ptr(arrs[0]), _as_ptr(arrs[1]), _as_ptr(arrs[2])))
        r = {"n": int(score[0]), "weight_sum": int(score[1]), "loss_pi": float(score[2]), "loss_v": float(score[3]), "kl": float(score[4]),
             "top1": float(score[5]), "sums": tuple(int(x) for x in sums)}
        if per_tuple or out is not None:
            r["ce"], r["se"], r["kl_rows"] = arrs
        return r

    def samples_holdout(self, share, seed, pis, zs, *, states=None, boards=None, out=None):
        """az_samples_holdout: the hold-out mask (bool [n]) of a window at share (a fraction; share_e6 = round(share * 1e6)) and seed: a
        function of the position alone, the same for a position and its mirror image.  out: a uint8 array or tensor to write into."""
        src, keep, n = self._tuples(pis, zs, states, boards, None)
        held = out if out is not None else np.full(n, 255, np.uint8)
        self._check(self._lib.az_samples_holdout(self._h, C.byref(src), int(round(float(share) * 1e6)), int(seed) & (2 ** 64 - 1), _as_ptr(held)))
        return held if out is not None else held.astype(bool)

    def train_set_validation(self, pis=None, zs=None, *, states=None, boards=None, weights=None):
        """az_net_train_set_validation: register (copy to the device) the set train() and train_samples() score at the end of every
        epoch; no arguments clear it."""
        if pis is None:
            self._check(self._lib.az_net_train_set_validation(self._h, None, None))
            return
        src, keep, n = self._tuples(pis, zs, states, boards, weights)
        self._check(self._lib.az_net_train_set_validation(self._h, C.byref(src), _as_ptr(keep[4])))

    def train_validation(self):
        """([(loss_pi, loss_v, kl, top1)] per epoch of the last train() / train_samples() with a validation set, best_epoch or -1)."""
        best = C.c_int32(-1)
        n = self._lib.az_net_train_validation(self._h, None, 0, None)
        out = np.zeros((n, 4), np.float64)
        self._lib.az_net_train_validation(self._h, _ptr(out), n, C.byref(best))
        return [tuple(float(x) for x in r) for r in out], int(best.value)

    def train_begin(self, prev_id):
        self._check(self._lib.az_net_train_begin(self._h, prev_id))

    def train_step(self, boards, pis, vs, mask_seed=0, apply=True, want_grads=False):
        """One optimisation step on an explicit batch -> ((loss_pi, loss_v), grads or None)."""
        b = np.ascontiguousarray(boards, dtype=np.float32)
        p = np.ascontiguousarray(pis, dtype=np.float32)
        v = np.ascontiguousarray(vs, dtype=np.float32)
        loss = np.zeros(2, np.float32)
        grads = np.zeros(self.net_param_count(), np.float32) if want_grads else None
        self._check(self._lib.az_net_train_step(self._h, _ptr(b), _ptr(p), _ptr(v), v.size, int(mask_seed), int(bool(apply)),
                                           _ptr(loss), _ptr(grads) if want_grads else None))
        return (float(loss[0]), float(loss[1])), grads

    def train_end(self, model_id):
        self._check(self._lib.az_net_train_end(self._h, model_id))

    def train_ema(self, model_id):
        """Store the averaged weights of "train_ema_decay_e9" (the last train_begin saw it > 0) under model_id."""
        self._check(self._lib.az_net_train_ema(self._h, model_id))

    def train_step_info(self):
        """(grad_norm, clip_scale, lr_t, applied steps since train_begin) of the last step; (-1, 1, ..) with clipping off."""
        out = np.zeros(4, np.float64)
        self._check(self._lib.az_net_train_step_info(self._h, _ptr(out)))
        return float(out[0]), float(out[1]), float(out[2]), int(out[3])

    def set_option(self, key, value):
        """az_set_option on this engine (keys: include/az_engine.h), e.g. set_option("net_fp8", 1): conv3 and conv4 of this engine's
        conv-net forwards on the FP8 (e4m3) matrix path -- a numerics class of its own, default off."""
        self._check(self._lib.az_set_option(self._h, key.encode(), int(value)))

    def set_search_stop(self, on):
        """az_search_stop_set (include/az_search_stop.h, default off): a temperature-0 search ends once its most visited root child leads
        the runner-up by more than the simulations still to come -- the move and pi are the full search's, counts and q those of the search
        as far as it ran.  Refused while a self-play session is open."""
        if not hasattr(self._lib, "az_search_stop_set"):
            raise RuntimeError("the loaded engine library has no az_search_stop_set (a build older than include/az_search_stop.h)")
        self._check(self._lib.az_search_stop_set(self._h, int(on)))

    def get_search_stop(self):
        if not hasattr(self._lib, "az_search_stop_get"):
            return 0
        v = C.c_int32(0)
        self._check(self._lib.az_search_stop_get(self._h, C.byref(v)))
        return int(v.value)

    def search_stop_stats(self, reset=False):
        """az_search_stop_stats: dict of the four counters over the finished calls (eligible_moves, stopped_moves, budgeted_sims,
        skipped_sims); reset clears them afterwards."""
        if not hasattr(self._lib, "az_search_stop_stats"):
            raise RuntimeError("the loaded engine library has no az_search_stop_stats (a build older than include/az_search_stop.h)")
        out = np.zeros(4, np.uint64)
        self._check(self._lib.az_search_stop_stats(self._h, _ptr(out), 1 if reset else 0))
        return dict(zip(("eligible_moves", "stopped_moves", "budgeted_sims", "skipped_sims"), (int(x) for x in out)))

    def set_eval_mirror(self, on):
        """The opt-in "eval_mirror" (include/az_engine.h, default off): every forward of a conv model of this engine is taken on the
        canonical one of the position and its left-right mirror image, and pi is un-mirrored for the asker -- the net's function becomes
        exactly mirror-equivariant, and a position and its mirror share one batch row and one evaluation-cache entry.  A numerics class
        of its own, like "net_fp8"; refused while a self-play session is open."""
        self.set_option("eval_mirror", 1 if on else 0)

    def set_root_noise(self, eps, alpha=1.0):
        """Dirichlet root noise of self-play and the tree calls (never the arena): prior <- (1 - eps) * prior + eps * eta,
        eta ~ Dirichlet(alpha) over the root's valid moves, once per get_action_prob.  eps = 0 switches it off (the default);
        the values travel as "root_noise_eps_e6" / "root_noise_alpha_e6" (include/az_engine.h)."""
        self.set_option("root_noise_alpha_e6", int(round(float(alpha) * 1e6)))
        self.set_option("root_noise_eps_e6", int(round(float(eps) * 1e6)))

    def set_playout_cap(self, sims, p_full=0.25):
        """Playout cap randomization of self-play (never the arena or the tree calls): a share p_full of an episode's moves is searched
        with the full num_sims, gets root noise if that is on and is recorded; every other move is searched with `sims` simulations and
        only played.  sims = 0 switches it off (the default); the values travel as "playout_cap_sims" / "playout_cap_full_e6"
        (include/az_engine.h)."""
        self.set_option("playout_cap_full_e6", int(round(float(p_full) * 1e6)))
        self.set_option("playout_cap_sims", int(sims))

    def set_forced_playouts(self, k, prune=False):
        """Forced playouts at the root and policy target pruning (KataGo) on every move root noise can apply to -- self-play and the tree
        calls, under a playout cap the full moves only, never the arena.  A visited root child with fewer than sqrt(k * prior * visits)
        visits wins the root's selection; with prune the recorded (and sampled) pi is formed from counts with those forced visits taken
        back out.  k = 0 switches both off (the default); the values travel as "forced_playouts_k_e6" / "policy_prune"
        (include/az_engine.h)."""
        self.set_option("policy_prune", 1 if prune else 0)
        self.set_option("forced_playouts_k_e6", int(round(float(k) * 1e6)))

    def set_gumbel(self, m, c_visit=50.0, c_scale=1.0):
        """Gumbel root search with sequential halving (Danihelka et al. 2022) on every move root noise can apply to -- lock-step self-play
        and az_tree_get_action_prob, under a playout cap the full moves only, never the arena or the slot calls.  The root samples at most
        m actions without replacement through Gumbel noise, spends the budget by sequential halving, plays the winner and records
        softmax(logits + sigma(completed Q)) as pi.  m = 0 switches it off (the default); the values travel as "gumbel_m" /
        "gumbel_c_visit_e6" / "gumbel_c_scale_e6" (include/az_engine.h)."""
        self.set_option("gumbel_c_visit_e6", int(round(float(c_visit) * 1e6)))
        self.set_option("gumbel_c_scale_e6", int(round(float(c_scale) * 1e6)))
        self.set_option("gumbel_m", int(m))

    def set_train_optim(self, weight_decay=0.0, clip_norm=0.0, lr_warmup_steps=0, lr_decay=0, lr_floor=0.0, ema_decay=0.0, lr_total_steps=0):
        """The opt-in optimiser rules of NNet::train, read by the next train() / train_begin(): decoupled AdamW weight decay, global
        gradient-norm clipping, linear warm-up with cosine (1) or linear (2) decay to lr_floor x lr, and an averaged shadow of the weights
        (train_ema).  Everything 0 (the default) switches them off; the values travel as "train_weight_decay_e9", "train_clip_norm_e6",
        "train_lr_warmup_steps", "train_lr_decay", "train_lr_floor_e6", "train_lr_total_steps" (the step entries only) and
        "train_ema_decay_e9" (include/az_engine.h)."""
        self.set_option("train_weight_decay_e9", int(round(float(weight_decay) * 1e9)))
        self.set_option("train_clip_norm_e6", int(round(float(clip_norm) * 1e6)))
        self.set_option("train_lr_warmup_steps", int(lr_warmup_steps))
        self.set_option("train_lr_decay", int(lr_decay))
        self.set_option("train_lr_floor_e6", int(round(float(lr_floor) * 1e6)))
        self.set_option("train_lr_total_steps", int(lr_total_steps))
        self.set_option("train_ema_decay_e9", int(round(float(ema_decay) * 1e9)))

    def set_arena_openings(self, plies):
        """Paired arena openings (never self-play or the tree calls): arena game g and its seat-swapped twin g + total/2 start from the
        same position, `plies` random quiet plies (even, 2 .. 12) played onto the pair's base -- the opening book's entry, start_board or
        the initial board -- and different from pair to pair.  0 switches the random plies off (the default); the value travels as
        "arena_opening_plies" (include/az_engine.h)."""
        self.set_option("arena_opening_plies", int(plies))

    def arena_set_opening_book(self, boards):
        """az_arena_set_opening_book: boards [n, 2] (first seat's stones, second seat's stones), first seat to move; pair p of every later
        arena() starts from entry p % n.  None or an empty list clears the book."""
        b = np.ascontiguousarray(np.zeros((0, 2)) if boards is None else boards, dtype=np.uint64).reshape(-1, 2)
        self._check(self._lib.az_arena_set_opening_book(self._h, _ptr(b) if len(b) else None, len(b)))

    def arena_get_openings(self, n_games):
        """Openings of the last arena(): (boards [n_games, 2] the position each game started from, len [n_games] the random plies played
        onto its base, moves [n_games, 12] those actions)."""
        boards = np.zeros((n_games, 2), np.uint64)
        ln = np.zeros(n_games, np.int32)
        moves = np.zeros((n_games, 12), np.uint8)
        self._check(self._lib.az_arena_get_openings(self._h, _ptr(boards), _ptr(ln), _ptr(moves)))
        return boards, ln, moves

    def selfplay_full_plies(self):
        """az_selfplay_get_full_plies: uint64 [n], bit `ply` of word i set when that ply of the i-th episode of the last selfplay() /
        selfplay_next() call was a full move, i.e. became a tuple (all plies when the playout cap is off)."""
        mask = np.zeros(self._sp_last_n, np.uint64)
        self._check(self._lib.az_selfplay_get_full_plies(self._h, _ptr(mask)))
        return mask

    def selfplay_search(self):
        """az_selfplay_get_search: (root_q [count], root_prior [count,7]) of the last selfplay() / selfplay_next(), tuple for tuple in the
        order of its pis and zs -- the root value R of the move and the root children's stored priors as the search used them.  Needs
        set_option("selfplay_record_search", 1) before that call."""
        n = getattr(self, "_sp_last_count", 0)
        q, prior = np.zeros(n, np.float32), np.zeros((n, ACTIONS), np.float32)
        self._check(self._lib.az_selfplay_get_search(self._h, _ptr(q), _ptr(prior)))
        return q, prior

    def root_noise_eta(self, states, game_ids, seed=0):
        """az_root_noise_eta: eta [n,7] the device sampler draws for root states [n,2] on the streams (seed, game_ids[i], stones),
        at the engine's current alpha."""
        s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 2)
        g = np.ascontiguousarray(game_ids, dtype=np.uint64).reshape(-1)
        assert g.shape[0] == s.shape[0]
        eta = np.empty((s.shape[0], ACTIONS), np.float32)
        self._check(self._lib.az_root_noise_eta(self._h, s.shape[0], seed, _ptr(g), _ptr(s), _ptr(eta)))
        return eta

    def gumbel_values(self, states, game_ids, seed=0, temp_is_zero=False):
        """az_gumbel_values: g [n,7] the device draws for root states [n,2] on the streams (seed, game_ids[i], stones); 0 for invalid
        actions, and everywhere when temp_is_zero."""
        s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 2)
        g = np.ascontiguousarray(game_ids, dtype=np.uint64).reshape(-1)
        assert g.shape[0] == s.shape[0]
        out = np.empty((s.shape[0], ACTIONS), np.float32)
        self._check(self._lib.az_gumbel_values(self._h, s.shape[0], seed, _ptr(g), _ptr(s), 1 if temp_is_zero else 0, _ptr(out)))
        return out

    # ---- stats ----
    def stats(self):
        s = az_stats()
        self._check(self._lib.az_get_stats(self._h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in az_stats._fields_}

    def reset_stats(self):
        self._check(self._lib.az_reset_stats(self._h))

    # ---- AsyncMcts ----
    def tree_create(self, n_games, reserve, num_sims, max_depth, model_id, cpuct, num_threads=1):
        return TreeBatch(self, n_games, reserve, num_sims, max_depth, model_id, cpuct, num_threads)

    def tree_selected(self, tree):
        """az_tree_get_selected of a TreeBatch (see TreeBatch.selected)."""
        return tree.selected()

    def reanalyse(self, num_sims, model_id, *, states=None, boards=None, game_ids=None, temp=1.0, seed=0, first_game_id=0, concurrent=0,
                  max_depth=1000, cpuct=1, reserve=1000000, num_sim_threads=1, out=None):
        """az_reanalyse (include/az_reanalyse.h): a fresh search of each of n stored positions (states [n,2] u64 or boards [n,2,6,7]
        f32; game_ids u64 [n], None = first_game_id + i) with model_id as it is now.  Row i is bit for bit what a one-tree
        get_action_prob says after reset(states[i]).  Arrays may be numpy arrays or torch tensors (host or device).  Returns a dict: pi
        [n,7], root_q [n], root_prior [n,7], counts u16 [n,7], q [n,7], selected i32 [n]; out = a dict of caller arrays or tensors to
        write into instead (a key that is missing is allocated, a key that is None is not asked for; pi is always returned)."""
        if not hasattr(self._lib, "az_reanalyse"):
            raise RuntimeError("the loaded engine library has no az_reanalyse (a build older than include/az_reanalyse.h)")
        if (states is None) == (boards is None):
            raise ValueError("states or boards, not both")
        if states is not None and not hasattr(states, "data_ptr"):
            states = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 2)
        if boards is not None and not hasattr(boards, "data_ptr"):
            boards = np.ascontiguousarray(boards, dtype=np.float32).reshape(-1, 2, 6, 7)
        n = int(len(states if states is not None else boards))
        if game_ids is not None and not hasattr(game_ids, "data_ptr"):
            game_ids = np.ascontiguousarray(game_ids, dtype=np.uint64).reshape(n)
        shapes = {"pi": ((n, ACTIONS), np.float32), "root_q": ((n,), np.float32), "root_prior": ((n, ACTIONS), np.float32),
                  "counts": ((n, ACTIONS), np.uint16), "q": ((n, ACTIONS), np.float32), "selected": ((n,), np.int32)}
        res = dict(out or {})
        for k, (shape, dt) in shapes.items():
            if k not in res:
                res[k] = np.zeros(shape, dt)
        if res["pi"] is None:
            raise ValueError("pi is always returned")
        p = az_reanalyse_params(concurrent, num_sims, max_depth, cpuct, model_id, num_sim_threads, float(temp), reserve,
                                int(seed) & (2 ** 64 - 1), int(first_game_id) & (2 ** 64 - 1))
        self._check(self._lib.az_reanalyse(self._h, C.byref(p), n, _as_ptr(states), _as_ptr(boards), _as_ptr(game_ids), _as_ptr(res["pi"]),
                                           _as_ptr(res["root_q"]), _as_ptr(res["root_prior"]), _as_ptr(res["counts"]), _as_ptr(res["q"]),
                                           _as_ptr(res["selected"])))
        return res

    # ---- Coach::execute_episode x many ----
    def selfplay(self, n_games, num_sims, model_id, seed=0, first_game_id=0, concurrent=0, temp_threshold=15,
                 max_depth=1000, cpuct=1, reserve=1000000, symmetries=True, want_boards=True, want_states=True,
                 record_evals=0, out=None, num_sim_threads=1):
        """Plays n_games episodes; returns dict(states, boards, pis, zs, game_len, moves, count).

        `out` may hold pre-allocated torch CUDA tensors / numpy arrays for states/boards/pis/zs
        (the library writes device or host memory alike)."""
        nsym = 2 if symmetries else 1
        cap = n_games * MAX_PLIES * nsym
        out = dict(out or {})
        if "pis" not in out:
            out["pis"] = np.zeros((cap, ACTIONS), np.float32)
        if "zs" not in out:
            out["zs"] = np.zeros(cap, np.float32)
        if want_states and "states" not in out:
            out["states"] = np.zeros((cap, 2), np.uint64)
        if want_boards and "boards" not in out:
            out["boards"] = np.zeros((cap, 2, 6, 7), np.float32)
        game_len = np.zeros(n_games, np.int32)
        moves = np.zeros((n_games, MAX_PLIES), np.uint8)
        p = az_selfplay_params(n_games, concurrent, num_sims, temp_threshold, max_depth, cpuct, model_id,
                               1 if symmetries else 0, reserve, seed, first_game_id, record_evals, num_sim_threads)
        s = az_samples(cap, 0, _as_ptr(out.get("states")), _as_ptr(out.get("boards")), _as_ptr(out["pis"]),
                       _as_ptr(out["zs"]), _ptr(game_len), _ptr(moves))
        self._check(self._lib.az_selfplay(self._h, C.byref(p), C.byref(s)))
        self._sp_last_n = n_games
        self._sp_last_count = int(s.count)
        n = int(s.count)
        res = {"count": n, "game_len": game_len, "moves": moves}
        for k in ("states", "boards", "pis", "zs"):
            if k in out:
                res[k] = out[k][:n]
        return res

    def selfplay_begin(self, n_games, num_sims, model_id, seed=0, first_game_id=0, concurrent=0, temp_threshold=15, max_depth=1000,
                       cpuct=1, reserve=1000000, symmetries=True, record_evals=0, num_sim_threads=1):
        """Opens a self-play session of n_games episodes (az_selfplay_begin): selfplay_next(k) then returns the next k episodes in id
        order while the slots they freed already play later ones."""
        p = az_selfplay_params(n_games, concurrent, num_sims, temp_threshold, max_depth, cpuct, model_id,
                               1 if symmetries else 0, reserve, seed, first_game_id, record_evals, num_sim_threads)
        self._check(self._lib.az_selfplay_begin(self._h, C.byref(p)))
        self._sp_sym = bool(symmetries)

    def selfplay_next(self, n_games, want_boards=True, want_states=True, out=None):
        """The next n_games episodes of the open session: the dict selfplay() returns for the same episodes."""
        nsym = 2 if self._sp_sym else 1
        cap = n_games * MAX_PLIES * nsym
        out = dict(out or {})
        if "pis" not in out:
            out["pis"] = np.zeros((cap, ACTIONS), np.float32)
        if "zs" not in out:
            out["zs"] = np.zeros(cap, np.float32)
        if want_states and "states" not in out:
            out["states"] = np.zeros((cap, 2), np.uint64)
        if want_boards and "boards" not in out:
            out["boards"] = np.zeros((cap, 2, 6, 7), np.float32)
        game_len = np.zeros(n_games, np.int32)
        moves = np.zeros((n_games, MAX_PLIES), np.uint8)
        s = az_samples(cap, 0, _as_ptr(out.get("states")), _as_ptr(out.get("boards")), _as_ptr(out["pis"]),
                       _as_ptr(out["zs"]), _ptr(game_len), _ptr(moves))
        self._check(self._lib.az_selfplay_next(self._h, n_games, C.byref(s)))
        self._sp_last_n = n_games
        self._sp_last_count = int(s.count)
        n = int(s.count)
        res = {"count": n, "game_len": game_len, "moves": moves}
        for k in ("states", "boards", "pis", "zs"):
            if k in out:
                res[k] = out[k][:n]
        return res

    def selfplay_end(self):
        self._check(self._lib.az_selfplay_end(self._h))

    def selfplay_get_evals(self, n_games, cap):
        cnt = np.zeros(n_games, np.int32)
        states = np.zeros((n_games, cap, 2), np.uint64)
        pis = np.zeros((n_games, cap, ACTIONS), np.float32)
        vs = np.zeros((n_games, cap), np.float32)
        self._check(self._lib.az_selfplay_get_evals(self._h, _ptr(cnt), _ptr(states), _ptr(pis), _ptr(vs)))
        return cnt, states, pis, vs

    # ---- position averaging ----
    def merge_samples(self, pis, zs, *, states=None, boards=None, canonical=False, want_boards=False):
        """az_samples_merge: one tuple per distinct position of n tuples, carrying the mean pi and the mean z of its copies, in order
        of first occurrence (include/az_engine.h).  The position comes from `states` [n,2], or from `boards` [n,2,6,7] when states is
        None; canonical merges a position with its left-right mirror image.  Inputs may be numpy arrays or torch tensors (host or
        device).  Returns dict(count, states, pis, zs, counts) as numpy arrays, plus boards with want_boards."""
        if (states is None) == (boards is None):
            raise ValueError("merge_samples takes states or boards, not both")
        n = int(len(zs))
        if not hasattr(pis, "data_ptr"):
            pis = np.ascontiguousarray(pis, dtype=np.float32).reshape(n, ACTIONS)
        if not hasattr(zs, "data_ptr"):
            zs = np.ascontiguousarray(zs, dtype=np.float32).reshape(n)
        if states is not None and not hasattr(states, "data_ptr"):
            states = np.ascontiguousarray(states, dtype=np.uint64).reshape(n, 2)
        if boards is not None and not hasattr(boards, "data_ptr"):
            boards = np.ascontiguousarray(boards, dtype=np.float32).reshape(n, 2, 6, 7)
        out = {"states": np.zeros((n, 2), np.uint64), "pis": np.zeros((n, ACTIONS), np.float32), "zs": np.zeros(n, np.float32),
               "counts": np.zeros(n, np.uint32)}
        if want_boards:
            out["boards"] = np.zeros((n, 2, 6, 7), np.float32)
        src = az_samples(n, n, _as_ptr(states), _as_ptr(boards), _as_ptr(pis), _as_ptr(zs), None, None)
        dst = az_samples(n, 0, _ptr(out["states"]), _ptr(out.get("boards")), _ptr(out["pis"]), _ptr(out["zs"]), None, None)
        self._check(self._lib.az_samples_merge(self._h, C.byref(src), MERGE_CANONICAL if canonical else 0, C.byref(dst), _ptr(out["counts"])))
        m = int(dst.count)
        res = {k: v[:m] for k, v in out.items()}
        res["count"] = m
        return res

    # ---- z/q value targets and surprise resampling ----
    def blend_z(self, zs, root_q, lam, out=None):
        """az_samples_blend_z: (1 - lam) * zs + lam * root_q in f32 (csrc/az_target.h); lam travels as lambda_e6.  Inputs may be numpy arrays
        or torch tensors (host or device); `out` may be either, zs itself included; without it a new numpy array is returned."""
        n = int(len(zs))
        if not hasattr(zs, "data_ptr"):
            zs = np.ascontiguousarray(zs, dtype=np.float32).reshape(n)
        if not hasattr(root_q, "data_ptr"):
            root_q = np.ascontiguousarray(root_q, dtype=np.float32).reshape(n)
        if len(root_q) != n:
            raise ValueError("blend_z: zs and root_q differ in length")
        if out is None:
            out = np.zeros(n, np.float32)
        self._check(self._lib.az_samples_blend_z(self._h, n, _as_ptr(zs), _as_ptr(root_q), int(round(float(lam) * 1e6)), _as_ptr(out)))
        return out

    def surprise(self, pis, zs, priors, share, seed, *, states=None, boards=None, want=True):
        """az_samples_surprise: tuple i repeated c_i times, c_i drawn around a weight of which a share `share` is in proportion to
        KL(pi_i || prior_i) and the rest uniform (include/az_engine.h).  The position comes from `states` [n,2] and/or `boards` [n,2,6,7];
        inputs may be numpy arrays or torch tensors (host or device).  Returns dict(counts, kl) and, with want, count and the expanded
        pis, zs and states / boards (whichever were given) as numpy arrays."""
        if states is None and boards is None:
            raise ValueError("surprise needs states or boards")
        n = int(len(zs))
        if not hasattr(pis, "data_ptr"):
            pis = np.ascontiguousarray(pis, dtype=np.float32).reshape(n, ACTIONS)
        if not hasattr(zs, "data_ptr"):
            zs = np.ascontiguousarray(zs, dtype=np.float32).reshape(n)
        if not hasattr(priors, "data_ptr"):
            priors = np.ascontiguousarray(priors, dtype=np.float32).reshape(n, ACTIONS)
        if states is not None and not hasattr(states, "data_ptr"):
            states = np.ascontiguousarray(states, dtype=np.uint64).reshape(n, 2)
        if boards is not None and not hasattr(boards, "data_ptr"):
            boards = np.ascontiguousarray(boards, dtype=np.float32).reshape(n, 2, 6, 7)
        res = {"counts": np.zeros(n, np.uint32), "kl": np.zeros(n, np.float32)}
        src = az_samples(n, n, _as_ptr(states), _as_ptr(boards), _as_ptr(pis), _as_ptr(zs), None, None)
        out, dst = {}, None
        if want:
            cap = 2 * n
            out = {"pis": np.zeros((cap, ACTIONS), np.float32), "zs": np.zeros(cap, np.float32)}
            if states is not None:
                out["states"] = np.zeros((cap, 2), np.uint64)
            if boards is not None:
                out["boards"] = np.zeros((cap, 2, 6, 7), np.float32)
            dst = az_samples(cap, 0, _ptr(out.get("states")), _ptr(out.get("boards")), _ptr(out["pis"]), _ptr(out["zs"]), None, None)
        self._check(self._lib.az_samples_surprise(self._h, C.byref(src), _as_ptr(priors), int(round(float(share) * 1e6)), int(seed) & ((1 << 64) - 1),
                                                  C.byref(dst) if dst is not None else None, _ptr(res["counts"]), _ptr(res["kl"])))
        if want:
            m = int(dst.count)
            res["count"] = m
            for k, v in out.items():
                res[k] = v[:m]
        return res

    # ---- exact endgame solver ----
    def solve(self, states, max_nodes=1 << 20, min_stones=0, tt_log2=12, max_lanes=0):
        """az_solve: every root action of n canonical positions [n,2] (numpy or torch, host or device).  Returns (move_values [n,7] int8,
        values [n] int8, nodes [n,7] uint32): the exact outcome for the side to move after the action (-1, 0, +1), SOLVE_ILLEGAL for an
        action that is not legal, SOLVE_UNKNOWN where the search passed max_nodes or the position has fewer than min_stones stones
        (include/az_engine.h)."""
        if not hasattr(states, "data_ptr"):
            states = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 2)
        n = int(len(states))
        mv, values, nodes = np.zeros((n, ACTIONS), np.int8), np.zeros(n, np.int8), np.zeros((n, ACTIONS), np.uint32)
        self._check(self._lib.az_solve(self._h, _as_ptr(states), n, max_nodes, min_stones, tt_log2, max_lanes, _ptr(mv), _ptr(values), _ptr(nodes)))
        return mv, values, nodes

    def move_quality(self, game_len, moves, start_boards=None, max_nodes=1 << 20, min_stones=0, tt_log2=12, max_lanes=0):
        """az_move_quality: the recorded games (game_len [n], moves [n,42] as arena_get_moves and selfplay return them; start_boards [n,2]
        as arena_get_openings returns them, None = the initial board) replayed and every move classed against the exact value of its
        position.  Returns (ply_class [n,42] uint8 of MQ_*, ply_value [n,42] int8)."""
        game_len = np.ascontiguousarray(game_len, dtype=np.int32).reshape(-1)
        n = int(len(game_len))
        moves = np.ascontiguousarray(moves, dtype=np.uint8).reshape(n, MAX_PLIES)
        if start_boards is not None:
            start_boards = np.ascontiguousarray(start_boards, dtype=np.uint64).reshape(n, 2)
        cls, val = np.zeros((n, MAX_PLIES), np.uint8), np.zeros((n, MAX_PLIES), np.int8)
        self._check(self._lib.az_move_quality(self._h, _ptr(start_boards), _ptr(game_len), _ptr(moves), n, max_nodes, min_stones, tt_log2, max_lanes,
                                              _ptr(cls), _ptr(val)))
        return cls, val

    # ---- arena::play_games ----
    def arena(self, num_games, num_sims, new_model_id, old_model_id, seed=0, max_depth=1000, cpuct=1,
              reserve=1000000, first_game=0, total_games=0, record_evals=0, num_sim_threads=1, start_board=None, allreduce_wld=False):
        """play_games: (W, L, D) for the new model + per-game results.  total_games > 0 plays the shard
        [first_game, first_game + num_games) of a total_games arena (seating / RNG by global game index).
        start_board = (first seat's stones, second seat's stones): play_games' `board` argument."""
        sb = (C.c_uint64 * 2)(*(int(x) for x in (start_board if start_board is not None else (0, 0))))
        p = az_arena_params(num_games, num_sims, max_depth, cpuct, new_model_id, old_model_id, reserve, seed,
                            first_game, total_games, record_evals, num_sim_threads, 0 if start_board is None else 1,
                            1 if allreduce_wld else 0, sb)
        wld = np.zeros(3, np.uint64)
        results = np.zeros(max(num_games, 1), np.int8)
        self._check(self._lib.az_arena(self._h, C.byref(p), _ptr(wld), _ptr(results)))
        return wld, results[: (num_games if total_games > 0 else 2 * (num_games // 2))]


    def arena_get_moves(self, n_games):
        """Move record of the last arena(): (game_len [n_games], moves [n_games, 42])."""
        game_len = np.zeros(n_games, np.int32)
        moves = np.zeros((n_games, MAX_PLIES), np.uint8)
        self._check(self._lib.az_arena_get_moves(self._h, _ptr(game_len), _ptr(moves)))
        return game_len, moves

    def tournament(self, model_ids, games_per_pair, num_sims, seed=0, max_depth=1000, cpuct=1, reserve=1000000, num_sim_threads=1):
        """az_tournament: one batched round robin of the K = len(model_ids) models, games_per_pair games (half per seating) for each of the
        P = K (K - 1) / 2 pairs (i, j), i < j, in lexicographic order.  Game g of pair p is bit for bit game g of
        arena(games_per_pair, num_sims, model_ids[i], model_ids[j], seed, ...) and has index p * games_per_pair + g.  Returns a dict:
        wld [K,K,3] uint64 (wld[i,j] = (W, L, D) from model i's side), results [P*n] int8 (+1: the first seat won), game_len [P*n] and
        moves [P*n,42] (the move record arena_get_moves returns afterwards).  Switch paired openings on first (set_arena_openings)."""
        ids = np.ascontiguousarray(model_ids, dtype=np.int32).reshape(-1)
        K, n = int(len(ids)), int(games_per_pair)
        games = max(K * (K - 1) // 2 * max(n, 0), 1)
        wld = np.zeros((K, K, 3), np.uint64)
        results = np.zeros(games, np.int8)
        self._check(self._lib.az_tournament(self._h, _ptr(ids), K, n, num_sims, max_depth, cpuct, num_sim_threads, reserve, seed,
                                            _ptr(wld), _ptr(results)))
        game_len, moves = self.arena_get_moves(games)
        return {"wld": wld, "results": results, "game_len": game_len, "moves": moves}

    def arena_get_evals(self, which, n_games, cap):
        """Eval log of the last arena(record_evals=cap): rows the trees of player `which` (0 new, 1 old) consumed, per game."""
        cnt = np.zeros(n_games, np.int32)
        states = np.zeros((n_games, cap, 2), np.uint64)
        pis = np.zeros((n_games, cap, ACTIONS), np.float32)
        vs = np.zeros((n_games, cap), np.float32)
        self._check(self._lib.az_arena_get_evals(self._h, which, _ptr(cnt), _ptr(states), _ptr(pis), _ptr(vs)))
        return cnt, states, pis, vs

    # ---- the collective of the sharded Coach loop (RCCL on the engine's stream) ----
    def comm_unique_id(self):
        buf = np.zeros(COMM_ID_BYTES, np.uint8)
        self._check(self._lib.az_comm_unique_id(self._h, _ptr(buf)))
        return buf

    def comm_local_id(self, world):
        """The 128-byte id of an IN-PROCESS communicator of `world` ranks: engines of this process that comm_init with it form one
        world without RCCL.  Each rank's collectives block until every rank has called them, so drive each engine from its own
        thread (ctypes releases the GIL during the call)."""
        buf = np.zeros(COMM_ID_BYTES, np.uint8)
        self._check(self._lib.az_comm_local_id(self._h, int(world), _ptr(buf)))
        return buf

    def comm_init(self, rank, world, unique_id):
        buf = np.ascontiguousarray(unique_id, np.uint8)
        assert buf.size == COMM_ID_BYTES
        self._check(self._lib.az_comm_init(self._h, rank, world, _ptr(buf)))
        self._comm_world = int(world)

    def comm_destroy(self):
        self._check(self._lib.az_comm_destroy(self._h))

    def gather_samples(self, states, pis, zs, dst=0, is_dst=True, capacity=0, out=None):
        """ONE gather of this rank's (s, pi, z) tuples to rank dst (-1: every rank receives); returns (states, pis, zs, counts) on a
        receiving rank, (None, None, None, counts) elsewhere.  counts has one entry per rank of the communicator.
        out = {"states", "pis", "zs"}: receive into these buffers (numpy arrays or torch tensors, host or device; capacity = their
        rows) instead of fresh host arrays -- the returned tuple then holds views of them."""
        n = int(len(zs))
        local = az_samples(n, n, _as_ptr(states), None, _as_ptr(pis), _as_ptr(zs), None, None)
        counts = np.zeros(max(1, getattr(self, "_comm_world", 1)), np.int64)
        if is_dst:
            if out is not None:
                gs, gp, gz = out["states"], out["pis"], out["zs"]
                capacity = int(gz.shape[0])
                g = az_samples(capacity, 0, _as_ptr(gs), None, _as_ptr(gp), _as_ptr(gz), None, None)
            else:
                gs, gp, gz = np.zeros((capacity, 2), np.uint64), np.zeros((capacity, ACTIONS), np.float32), np.zeros(capacity, np.float32)
                g = az_samples(capacity, 0, _ptr(gs), None, _ptr(gp), _ptr(gz), None, None)
            self._check(self._lib.az_gather_samples(self._h, C.byref(local), dst, C.byref(g), _ptr(counts)))
            m = int(g.count)
            return gs[:m], gp[:m], gz[:m], counts
        self._check(self._lib.az_gather_samples(self._h, C.byref(local), dst, None, _ptr(counts)))
        return None, None, None, counts

    def allreduce_u64(self, values):
        v = np.ascontiguousarray(values, np.uint64).copy()
        self._check(self._lib.az_allreduce_u64(self._h, _ptr(v), v.size))
        return v


class TreeBatch:
    """n_games x AsyncMcts::default(..) rooted at the initial board (src/async_mcts.rs:27-48)."""

    def __init__(self, engine, n_games, reserve, num_sims, max_depth, model_id, cpuct, num_threads=1):
        self.engine = engine
        self.n_games = n_games
        h = C.c_void_p()
        engine._check(engine._lib.az_tree_create(engine._h, n_games, reserve, num_sims, num_threads, max_depth, model_id, cpuct, C.byref(h)))
        self._h = h
        self._log_cap = 0
        engine._trees.add(self)

    def close(self):
        if self._h and self.engine._h:
            self.engine._lib.az_tree_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_action_prob(self, states, temp, seed=0, first_game_id=0):
        """states [G,2] uint64 canonical bitboards -> (pi [G,7] f32, counts [G,7] u16, q [G,7] f32)."""
        s = np.ascontiguousarray(states, dtype=np.uint64).reshape(self.n_games, 2)
        pi = np.empty((self.n_games, ACTIONS), np.float32)
        counts = np.empty((self.n_games, ACTIONS), np.uint16)
        q = np.empty((self.n_games, ACTIONS), np.float32)
        self.engine._check(self.engine._lib.az_tree_get_action_prob(self._h, _ptr(s), temp, seed, first_game_id, _ptr(pi),
                                                        _ptr(counts), _ptr(q)))
        return pi, counts, q

    def selected(self):
        """az_tree_get_selected: int32 [G], the selected action of each tree's last get_action_prob when that was a Gumbel move
        ("gumbel_m" > 0), else -1."""
        out = np.zeros(self.n_games, np.int32)
        self.engine._check(self.engine._lib.az_tree_get_selected(self._h, _ptr(out)))
        return out

    def reset(self, root_states=None):
        """AsyncMcts::from_state: re-root every tree (None = the initial board)."""
        s = None if root_states is None else np.ascontiguousarray(root_states, dtype=np.uint64).reshape(self.n_games, 2)
        self.engine._check(self.engine._lib.az_tree_reset(self._h, _ptr(s)))

    def record_evals(self, cap):
        self.engine._check(self.engine._lib.az_tree_record_evals(self._h, cap))
        self._log_cap = cap

    def get_evals(self):
        cap = self._log_cap
        cnt = np.zeros(self.n_games, np.int32)
        states = np.zeros((self.n_games, cap, 2), np.uint64)
        pis = np.zeros((self.n_games, cap, ACTIONS), np.float32)
        vs = np.zeros((self.n_games, cap), np.float32)
        self.engine._check(self.engine._lib.az_tree_get_evals(self._h, _ptr(cnt), _ptr(states), _ptr(pis), _ptr(vs)))
        return cnt, states, pis, vs

    def node_counts(self):
        out = np.zeros(self.n_games, np.uint32)
        self.engine._check(self.engine._lib.az_tree_node_counts(self._h, _ptr(out)))
        return out

    # ---- shared tree batch (az_tree_share): one slot per host thread, the threads' calls coalesced into batched searches ----
    def share(self, window_us=0):
        """Turn the batch into a shared one; from now on only the slot_* calls drive it.  ctypes releases the GIL during a
        call, so threading.Threads calling slot_get_action_prob really wait for (and run) batches concurrently."""
        self.engine._check(self.engine._lib.az_tree_share(self._h, window_us))

    def slot_acquire(self):
        """AsyncMcts::default on a free slot (its tree starts at the initial board); raises AzError(AZ_ERR_CAPACITY) when all are held."""
        slot = C.c_int32(-1)
        st = self.engine._lib.az_tree_slot_acquire(self._h, C.byref(slot))
        if st != AZ_OK:
            raise AzError(st, "az_tree_slot_acquire")
        return slot.value

    def slot_release(self, slot):
        st = self.engine._lib.az_tree_slot_release(self._h, slot)
        if st != AZ_OK:
            raise AzError(st, "az_tree_slot_release: slot out of range or not held")

    def slot_get_action_prob(self, slot, state, temp, seed=0, game_id=0):
        """get_action_prob on one held slot: state (mine, theirs) canonical -> (pi [7] f32, counts [7] u16, q [7] f32).
        Blocks until the batch that carries the request has run."""
        s = np.ascontiguousarray(state, dtype=np.uint64).reshape(2)
        pi = np.empty(ACTIONS, np.float32)
        counts = np.empty(ACTIONS, np.uint16)
        q = np.empty(ACTIONS, np.float32)
        st = self.engine._lib.az_tree_slot_get_action_prob(self._h, slot, _ptr(s), temp, seed, game_id, _ptr(pi), _ptr(counts), _ptr(q))
        if st != AZ_OK:
            raise AzError(st, self.slot_error(slot))
        return pi, counts, q

    def slot_error(self, slot):
        msg = self.engine._lib.az_tree_slot_error(self._h, slot)
        return msg.decode() if msg else ""

    def share_stats(self):
        """{batches, requests, largest, by_window} since share()."""
        out = np.zeros(4, np.uint64)
        self.engine._check(self.engine._lib.az_tree_share_stats(self._h, _ptr(out)))
        return dict(zip(("batches", "requests", "largest", "by_window"), (int(x) for x in out)))


# ---- host-side helpers on canonical bitboards (mirror of the Game trait for Connect Four) ----
def rating_fit(wld, prior_games=2.0):
    """az_rating_fit: Bradley-Terry ratings (a draw = half a win, Hunter's MM iteration) from a result matrix wld [K,K,3] as
    Engine.tournament returns it.  Needs no engine and no GPU.  Returns (elo [K] with mean 0, elo_se [K] -- the diagonal Fisher
    approximation --, sweeps).  prior_games virtual games are added to every pair, half won by each side; 2 is the recommended value."""
    wld = np.ascontiguousarray(wld, dtype=np.uint64)
    if wld.ndim != 3 or wld.shape[0] != wld.shape[1] or wld.shape[2] != 3:
        raise ValueError("wld must be [K, K, 3]")
    K = int(wld.shape[0])
    elo, se, sweeps = np.zeros(K, np.float64), np.zeros(K, np.float64), C.c_int32(0)
    st = _lib.az_rating_fit(_ptr(wld), K, float(prior_games), _ptr(elo), _ptr(se), C.byref(sweeps))
    if st != AZ_OK:
        raise AzError(st, "az_rating_fit: K outside 2 .. 16, or a negative or non-finite prior_games")
    return elo, se, int(sweeps.value)


def c4_play(mine, theirs, a):
    """get_next_state(1, a) then get_canonical_form(next_player) (connect_four_game.rs:90-103, :198-203)."""
    mask = mine | theirs
    nb = (mask + (1 << (a * 7))) & (0x3F << (a * 7))
    return theirs, mine | nb


def c4_features(mine, theirs):
    """to_features: [2,6,7] f32 (connect_four_game.rs:219-237, NCHW per repair S8)."""
    f = np.zeros((2, 6, 7), np.float32)
    for r in range(6):
        for c in range(7):
            bit = 1 << (c * 7 + (5 - r))
            if mine & bit:
                f[0, r, c] = 1.0
            if theirs & bit:
                f[1, r, c] = 1.0
    return f
