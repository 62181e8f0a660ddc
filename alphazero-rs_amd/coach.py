"""Coach::learn around the MI355X engine -- SURVEY.md section 8(f1, f3).

Mirrors src/coach.rs: `Coach.setup` takes the reference's 15 parameters (src/coach.rs:38-54) with the same
meaning, `learn` runs the iteration loop of src/coach.rs:169-396: self-play episodes -> replay window
(max_queue_length / max_history_length) -> save examples -> [merge duplicate positions, opt-in] -> shuffle -> NNet::train -> arena of new vs old ->
accept iff nwins + pwins > 0 and nwins / (nwins + pwins) >= update_threshold (:383-390).  Self-play and the arena
are ONE engine call each (az_selfplay / az_arena); episodes shard across ranks by global game id when a process
group is active and the tuples are gathered once per iteration (alphazero-rs_amd/dist.py).

NNet::train is the engine's own (az_net_train, csrc/az_train.hip) unless a `trainer` object is passed (the PyTorch
autograd restatement of alphazero-rs_amd/trainer.py: what the CPU tests use).  Several ranks are REPLICAS for training:
every rank trains on the same gathered samples with the same seeds and, the kernels being deterministic, ends with the
same weights -- no gradient exchange.
The C++ host (include/az_host.hpp `Coach`) runs the same sequence with the same seeds and writes the same files.

On-disk formats (the reference's are bincode / TF checkpoints, src/coach.rs:159-167 with defect A14; these are the
build's own, documented here):
  <dir>/<iter>.examples   "AZEX0001": char magic[8]; int64 H; int64 lens[H] (samples per history entry);
                          f32 boards[N][2][6][7]; f32 pis[N][7]; f32 vs[N] -- the whole `history` deque, oldest first
  <dir>/<model_id>.aznet  weights file of az_net_save: the initial model and every candidate
  <dir>/coach.state       text "iteration model_id\n": the last finished iteration and the ACCEPTED model id after its gate
                          (a rejected candidate leaves its <id+1>.aznet behind; the state file says which id is live)
Resume picks the largest numeric stem, as Coach::setup does (:55-81); non-numeric files are ignored instead of
panicking; when coach.state names a model whose .aznet exists it is loaded into that engine slot, so iteration k+1 of a
restarted run is byte-identical to an uninterrupted one.
"""
import collections
import contextlib
import os
import time

import numpy as np


class Coach:
    def __init__(self):
        raise TypeError("use Coach.setup(...)")

    @classmethod
    def setup(cls, engine, checkpoint_directory, mcts_reserve_size, update_threshold, temp_threshold,
              max_history_length, max_queue_length, inference_batch_size, num_episode_threads, num_arena_games,
              num_iters, num_eps, num_sims, num_sim_threads, max_depth, cpuct, trainer=None, group=None, log=print):
        self = object.__new__(cls)
        if num_sims % inference_batch_size != 0:                      # assert!, src/coach.rs:83
            raise ValueError("num_sims % inference_batch_size != 0")
        if num_sim_threads < 1 or num_sims % num_sim_threads != 0:    # assert!, src/async_mcts.rs:192
            raise ValueError("num_sims % num_sim_threads != 0")
        self.num_sim_threads = num_sim_threads    # > 1: several simulations in flight per tree (the engine's lock-step schedule)
        self.engine, self.trainer, self.group, self.log = engine, trainer, group, log
        self.dir = str(checkpoint_directory)
        self.mcts_reserve_size, self.update_threshold, self.temp_threshold = mcts_reserve_size, update_threshold, temp_threshold
        self.max_history_length, self.max_queue_length = max_history_length, max_queue_length
        self.num_episode_threads = num_episode_threads    # = concurrent game slots on the GPU (rayon pool size, :202-205)
        self.num_arena_games, self.num_iters, self.num_eps, self.num_sims = num_arena_games, num_iters, num_eps, num_sims
        self.max_depth, self.cpuct = max_depth, cpuct
        # NET_CLASS_FP8 (engine.py): every iteration pins the playing model to fp8 before az_selfplay and both arena models to bf16
        # before az_arena; training is untouched.  NET_CLASS_ENGINE (-1, the default): no class call at all
        self.selfplay_class = -1
        # Dirichlet root noise of the episodes (Engine.set_root_noise): switched on before every az_selfplay and off again behind it, so
        # nothing else the engine is used for sees it (the arena never does anyway).  eps 0 (the default): the engine is never asked
        self.root_noise_eps, self.root_noise_alpha = 0.0, 1.0
        # Playout cap randomization of the episodes (Engine.set_playout_cap): switched on before every az_selfplay and off again behind it,
        # exactly as the root noise is.  sims 0 (the default): the engine is never asked.  An iteration then yields the full moves' tuples only
        self.playout_cap_sims, self.playout_cap_full = 0, 0.25
        # Forced playouts and policy target pruning of the episodes (Engine.set_forced_playouts): switched on before every az_selfplay and
        # off again behind it, exactly as the playout cap is.  k 0 (the default): the engine is never asked
        self.forced_playouts_k, self.policy_prune = 0.0, False
        # Gumbel root search with sequential halving of the episodes (Engine.set_gumbel): switched on before every az_selfplay and off again
        # behind it, exactly as the forced playouts are (the engine refuses the two together).  m 0 (the default): the engine is never asked
        self.gumbel_m, self.gumbel_c_visit, self.gumbel_c_scale = 0, 50.0, 1.0
        # Paired openings of the gate (Engine.set_arena_openings): switched on before the iteration's az_arena and off again behind it,
        # exactly as the forced playouts are around self-play.  0 (the default): the engine is never asked
        self.arena_opening_plies = 0
        # "eval_mirror" (Engine.set_eval_mirror): set ONCE at the start of learn() for the whole loop -- the episodes and the arena gate both
        # run under the mirror-canonical function F, so the gate compares like with like.  False (the default): the engine is never asked
        self.eval_mirror = False
        # The decided-move stop (Engine.set_search_stop; include/az_search_stop.h): set ONCE at the start of learn()
        # for the whole loop -- the episodes' temperature-0 moves and every move of the arena gate end once they can no longer change.
        # False (the default): the engine is never asked
        self.search_stop = False
        # Position averaging (Engine.merge_samples): every iteration's concatenated window is merged to one tuple per distinct position --
        # mean pi, mean z -- before the shuffle, so the shuffle and NNet::train see the merged set; `history` and the <iter>.examples files
        # stay raw (resume is unaffected, a later iteration may merge differently).  merge_canonical also merges a position with its
        # mirror image: the window already holds both orientations (symmetries are expanded before it is merged) and nothing expands
        # them again, so the net then trains on the CANONICAL orientation of every position only -- half the set, and no mirrored board
        # unless it is the canonical one; meant to go with eval_mirror, which evaluates on that orientation.  False (the default): the
        # engine is never asked
        self.merge_positions, self.merge_canonical = False, False
        # merge_weighted (requires merge_positions): the merge's multiplicities are kept, shuffled with their tuples, and NNet::train draws
        # every batch row in proportion to them (Engine.train_samples, from the merged STATES: no feature planes are made) -- the raw
        # window's distribution at the merged set's size and step count; under merge_canonical rows are mirrored at random, so the net
        # sees both orientations again.  The report gains samples_weight, the sum of the multiplicities (= samples_raw).  Files on disk
        # stay raw.  False (the default): the counts are dropped and az_net_train runs as before
        self.merge_weighted = False
        # The optimiser rules of NNet::train (Engine.set_train_optim): decoupled weight decay, gradient-norm clipping, warm-up and decay of
        # the learning rate (lr_decay 0 none / 1 cosine / 2 linear, over the call's own steps) and an averaged shadow of the weights, set
        # before the iteration's one az_net_train and cleared behind it.  With ema_decay > 0 the candidate -- what the arena gates, what
        # is saved as <id>.aznet and what the next iteration trains from -- is the averaged model (Engine.train_ema).  All 0 (the
        # default): the engine is never asked
        self.weight_decay, self.clip_norm, self.lr_warmup_steps, self.lr_decay, self.lr_floor, self.ema_decay = 0.0, 0.0, 0, 0, 0.0, 0.0
        # Move-quality report (Engine.move_quality): after every iteration's arena its games are replayed, every position with at least
        # solve_min_stones stones is solved exactly (budget solve_max_nodes per position and action) and the move played there classed; the
        # tally per model goes into the report ("quality") and one log line.  It decides nothing: the gate, the checkpoints, the .examples
        # files and coach.state are those of a run without it.  0 (the default): the engine is never asked
        self.solve_min_stones, self.solve_max_nodes = 0, 1 << 20
        # Search statistics as targets (Engine.blend_z / Engine.surprise; csrc/az_target.h).  Either one switches "selfplay_record_search" on
        # before every az_selfplay and off again behind it.  value_target_q (0 .. 1): right behind self-play the rank's own zs become
        # (1 - q) * z + q * R, R the root value of the tuple's search -- before any gather, so the result does not depend on the world size.
        # surprise_share (0 .. 1): the rank's own tuples are replaced by Engine.surprise's resampling (seed = seed + iteration), tuple i
        # repeated c_i times with a share surprise_share of the weight in proportion to KL(pi || root prior) -- before the gather and the
        # symmetry expansion; refused with a world above 1 (the normalisation would be per shard).  History, the .examples files, the merge
        # and the trainers see ordinary tuples; merge_positions + merge_weighted turn the duplicates back into draw weights.  Both 0 (the
        # default): the engine is never asked
        self.value_target_q, self.surprise_share = 0.0, 0.0
        # Held-out validation (Engine.samples_holdout / train_set_validation; csrc/az_score.h).  validation_share (0 .. 1): every iteration
        # the assembled window is split by the hold-out rule BEFORE merge and shuffle, with learn()'s constant seed -- a function of the
        # position alone, so a position (and its mirror image) is on the same side in every iteration; the rest is trained on, the held-out
        # part is registered raw and scored at the end of every epoch.  The report gains val_n, val_loss_pi, val_loss_v, val_top1 (one
        # entry per epoch) and best_epoch.  keep_best stores the best epoch's weights, patience > 0 stops after that many epochs without a
        # new best ("train_keep_best", "train_patience").  `history` and the .examples files keep every tuple.  The engine's trainer only.
        # 0 (the default): the engine is never asked and reports and files are what they were
        self.validation_share, self.keep_best, self.patience = 0.0, False, 0
        # Reanalyse (Engine.reanalyse; include/az_reanalyse.h).  reanalyse_sims > 0: every iteration, once the new
        # window is appended and the oldest dropped and BEFORE the .examples file is written, the pi of every tuple of every older history
        # entry is replaced by a fresh search of reanalyse_sims simulations with the current model in its self-play class: temp 1, seed +
        # iteration, game ids reanalyse_first_game_id(iteration, entry) + tuple, the Coach's forced playouts / Gumbel rule on, root noise off,
        # the playout cap untouched.  z is kept; with value_target_q > 0 the older entries' z is blended with the fresh root value.  The
        # file holds what was trained on, so a resumed run is byte-identical.  The report gains t_reanalyse and reanalysed.  Every rank holds
        # the whole history and runs the same deterministic calls.  0 (the default): the engine is never asked, files are what they were
        self.reanalyse_sims = 0
        self.history = collections.deque()
        self.start_iteration = 0
        os.makedirs(self.dir, exist_ok=True)
        stems = [int(f[:-9]) for f in os.listdir(self.dir) if f.endswith(".examples") and f[:-9].isdigit()]
        self.model_id = 0
        if stems:                                                      # src/coach.rs:55-81
            it = max(stems)
            self.history.extend(load_examples(os.path.join(self.dir, f"{it}.examples")))
            self.start_iteration = it + 1
            st = read_state(self.dir)
            if st is not None and st[0] == it:                         # the live model of the run being resumed
                self.model_id = st[1]
                path = os.path.join(self.dir, f"{self.model_id}.aznet")
                if os.path.exists(path):
                    engine.net_load(self.model_id, path)
        return self

    # ---- rank helpers -------------------------------------------------------------------------------------
    def _world(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(self.group), dist.get_world_size(self.group)
        return 0, 1

    def save_train_examples(self, iteration):
        """src/coach.rs:159-167 (A14 repaired: <dir>/<iter>.examples, not an absolute path)."""
        path = os.path.join(self.dir, f"{iteration}.examples")
        save_examples(path, self.history)
        return path

    @staticmethod
    @contextlib.contextmanager
    def _scoped(active, apply, clear):
        """An engine option that holds for one block only: apply() before it when `active`, clear() behind it (also when the block
        raises).  Not active: the engine is never asked."""
        if active:
            apply()
        try:
            yield
        finally:
            if active:
                clear()

    def _selfplay_root_noise(self):
        return self._scoped(self.root_noise_eps > 0, lambda: self.engine.set_root_noise(self.root_noise_eps, self.root_noise_alpha),
                            lambda: self.engine.set_root_noise(0.0, self.root_noise_alpha))

    def _selfplay_playout_cap(self):
        return self._scoped(self.playout_cap_sims > 0, lambda: self.engine.set_playout_cap(self.playout_cap_sims, self.playout_cap_full),
                            lambda: self.engine.set_playout_cap(0, self.playout_cap_full))

    def _selfplay_forced_playouts(self):
        return self._scoped(self.forced_playouts_k > 0, lambda: self.engine.set_forced_playouts(self.forced_playouts_k, self.policy_prune),
                            lambda: self.engine.set_forced_playouts(0.0, False))

    def _selfplay_gumbel(self):
        return self._scoped(self.gumbel_m > 0, lambda: self.engine.set_gumbel(self.gumbel_m, self.gumbel_c_visit, self.gumbel_c_scale),
                            lambda: self.engine.set_gumbel(0))

    def _selfplay_record_search(self):
        return self._scoped(self.value_target_q > 0 or self.surprise_share > 0, lambda: self.engine.set_option("selfplay_record_search", 1),
                            lambda: self.engine.set_option("selfplay_record_search", 0))

    def _train_optim(self):
        on = self.weight_decay > 0 or self.clip_norm > 0 or self.lr_warmup_steps > 0 or self.lr_decay != 0 or self.ema_decay > 0
        return self._scoped(on, lambda: self.engine.set_train_optim(self.weight_decay, self.clip_norm, self.lr_warmup_steps, self.lr_decay,
                                                                    self.lr_floor, self.ema_decay),
                            lambda: self.engine.set_train_optim())

    def _train_validation(self, active):
        def apply():
            self.engine.set_option("train_keep_best", 1 if self.keep_best else 0)
            self.engine.set_option("train_patience", int(self.patience))

        def clear():
            self.engine.set_option("train_keep_best", 0)
            self.engine.set_option("train_patience", 0)
            self.engine.train_set_validation()
        return self._scoped(active, apply, clear)

    def _arena_openings(self):
        return self._scoped(self.arena_opening_plies > 0, lambda: self.engine.set_arena_openings(self.arena_opening_plies),
                            lambda: self.engine.set_arena_openings(0))

    def reanalyse_history(self, model_id, iteration, seed):
        """Coach.reanalyse_sims: re-search every history entry but the newest (csrc/az_reanalyse.h states the rule; include/az_host.hpp
        Coach::reanalyse_history is the other host).  Returns the tuples re-searched."""
        if self.selfplay_class != -1:
            self.engine.net_set_class(model_id, self.selfplay_class)
        done = 0
        with self._selfplay_forced_playouts(), self._selfplay_gumbel():
            for hi in range(reanalyse_entries(len(self.history))):
                boards, pis, vs = self.history[hi]
                if vs.shape[0] == 0:
                    continue
                want = {"counts": None, "q": None, "selected": None, "root_prior": None}
                r = self.engine.reanalyse(self.reanalyse_sims, model_id, boards=boards, temp=1.0, seed=seed + iteration,
                                          first_game_id=reanalyse_first_game_id(iteration, hi), concurrent=self.num_episode_threads,
                                          max_depth=self.max_depth, cpuct=self.cpuct, reserve=self.mcts_reserve_size,
                                          num_sim_threads=self.num_sim_threads, out=want)
                if self.value_target_q > 0:
                    vs = self.engine.blend_z(vs, r["root_q"], self.value_target_q)
                self.history[hi] = (boards, r["pi"], vs)
                done += int(vs.shape[0])
        return done

    def execute_episodes(self, model_id, iteration, seed):
        """The self-play fan-out of src/coach.rs:241-272: num_eps x execute_episode, sharded by global game id."""
        from . import dist as azdist
        rank, world = self._world()
        if not (0.0 <= self.value_target_q <= 1.0 and 0.0 <= self.surprise_share <= 1.0):
            raise ValueError("value_target_q and surprise_share must be in 0 .. 1")
        if self.surprise_share > 0 and world > 1:
            raise ValueError("surprise_share needs a world of 1: the weights would be normalised per shard")
        lo, hi = azdist.shard_range(self.num_eps, rank, world)
        first = iteration * self.num_eps
        if hi > lo:
            with self._selfplay_root_noise(), self._selfplay_playout_cap(), self._selfplay_forced_playouts(), self._selfplay_gumbel(), \
                    self._selfplay_record_search():
                r = self.engine.selfplay(n_games=hi - lo, num_sims=self.num_sims, model_id=model_id, seed=seed,
                                         first_game_id=first + lo, concurrent=min(self.num_episode_threads, hi - lo),
                                         temp_threshold=self.temp_threshold, max_depth=self.max_depth, cpuct=self.cpuct,
                                         reserve=self.mcts_reserve_size, symmetries=False, want_boards=False,
                                         num_sim_threads=self.num_sim_threads)
                if self.value_target_q > 0 or self.surprise_share > 0:
                    root_q, root_prior = self.engine.selfplay_search()
            states, pis, zs = r["states"], r["pis"], r["zs"]
            if self.value_target_q > 0:                                 # a blended z is still a z
                zs = self.engine.blend_z(zs, root_q, self.value_target_q)
            if self.surprise_share > 0:                                 # a resampled set is still a set of tuples
                sp = self.engine.surprise(pis, zs, root_prior, self.surprise_share, seed + iteration, states=states)
                states, pis, zs = sp["states"], sp["pis"], sp["zs"]
        else:
            states, pis, zs = np.zeros((0, 2), np.uint64), np.zeros((0, 7), np.float32), np.zeros(0, np.float32)
        if world > 1:
            import torch
            import torch.distributed as tdist
            dev = torch.device("cuda", torch.cuda.current_device()) if tdist.get_backend(self.group) == "nccl" else torch.device("cpu")
            packed = azdist.pack_samples(torch.from_numpy(states.view(np.int64)).to(dev), torch.from_numpy(pis).to(dev),
                                         torch.from_numpy(zs).to(dev))
            counts = torch.zeros(world, dtype=torch.int64, device=dev)
            tdist.all_gather_into_tensor(counts, torch.tensor([packed.shape[0]], dtype=torch.int64, device=dev), group=self.group)
            cmax = int(counts.max())
            padded = torch.zeros((cmax, azdist.TUPLE_WORDS), dtype=torch.int32, device=dev)
            padded[: packed.shape[0]] = packed
            allp = torch.zeros((world * cmax, azdist.TUPLE_WORDS), dtype=torch.int32, device=dev)
            tdist.all_gather_into_tensor(allp, padded, group=self.group)        # every rank trains: all-gather
            allp = torch.cat([allp[r * cmax: r * cmax + int(counts[r])] for r in range(world)])
            s, p, z = azdist.unpack_samples(allp)
        else:
            import torch
            s, p, z = torch.from_numpy(states.view(np.int64)), torch.from_numpy(pis), torch.from_numpy(zs)
        from . import dist as azd
        s2, p2, z2 = azd.expand_symmetries(s.cpu(), p.cpu(), z.cpu())           # get_symmetries at the destination
        boards = states_to_boards(s2.numpy().view(np.uint64))
        return boards, p2.numpy(), z2.numpy()

    def learn(self, skip_first_play=False, seed=0, model_id=None):
        """src/coach.rs:169-396.  Engine model slots: `model_id` is the current net (default: the resumed run's live
        model, else 0), `model_id + 1` the candidate.  Returns a list of per-iteration dicts (wins, accepted, losses)."""
        rank, world = self._world()
        report = []
        if model_id is None:
            model_id = self.model_id
        first = os.path.join(self.dir, f"{model_id}.aznet")
        if rank == 0 and not os.path.exists(first):
            self.engine.net_save(model_id, first)                       # the run's initial model: what a restart would load
        free = getattr(self.engine, "net_free", None)
        if self.eval_mirror:
            self.engine.set_eval_mirror(True)
        if self.search_stop:
            self.engine.set_search_stop(True)
        for iteration in range(self.start_iteration, self.start_iteration + self.num_iters):
            t_play = t_train = t_arena = 0.0
            boards, pis, vs = np.zeros((0, 2, 6, 7), np.float32), np.zeros((0, 7), np.float32), np.zeros(0, np.float32)
            if not skip_first_play or iteration > self.start_iteration:
                t0 = time.perf_counter()
                if self.selfplay_class != -1:
                    self.engine.net_set_class(model_id, self.selfplay_class)
                boards, pis, vs = self.execute_episodes(model_id, iteration, seed)
                t_play = time.perf_counter() - t0
                if vs.shape[0] > self.max_queue_length:                 # :275-277: keep the newest max_queue_length
                    boards, pis, vs = boards[-self.max_queue_length:], pis[-self.max_queue_length:], vs[-self.max_queue_length:]
            self.history.append((boards, pis, vs))                      # :282: pushed even when the play was skipped (empty entry)
            if len(self.history) > self.max_history_length:             # :285-288
                self.history.popleft()
            if self.reanalyse_sims > 0:                                 # before the save: a resumed run reads what this one trained on
                t0 = time.perf_counter()
                reanalysed = self.reanalyse_history(model_id, iteration, seed)
                t_reanalyse = time.perf_counter() - t0
            if rank == 0:
                self.save_train_examples(iteration)                     # :291-293
            allb = np.concatenate([h[0] for h in self.history])
            allp = np.concatenate([h[1] for h in self.history])
            allv = np.concatenate([h[2] for h in self.history])
            assert allv.shape[0] > 0                                    # :305
            samples_raw = int(allv.shape[0])
            val_n = 0
            if self.validation_share > 0:                               # the split: before merge and shuffle, by the position alone
                if not 0.0 < self.validation_share < 1.0:
                    raise ValueError("validation_share must be in 0 .. 1 (exclusive)")
                if self.trainer is not None:
                    raise ValueError("validation_share needs the engine's trainer")
                held = np.asarray(self.engine.samples_holdout(self.validation_share, seed, allp, allv, boards=allb), bool)
                val_n = int(held.sum())
                if val_n == samples_raw:
                    raise ValueError("validation_share holds the whole window out")
                if val_n > 0:
                    self.engine.train_set_validation(allp[held], allv[held], boards=allb[held])
                    allb, allp, allv = allb[~held], allp[~held], allv[~held]
            elif self.keep_best or self.patience:
                raise ValueError("keep_best and patience need validation_share > 0")
            t_merge = None
            if self.merge_weighted and not self.merge_positions:
                raise ValueError("merge_weighted requires merge_positions")
            weighted = self.merge_weighted
            on_engine = weighted and self.trainer is None               # states in, states out: no planes
            mult = None
            if self.merge_positions:                                    # one tuple per distinct position of the window
                t0 = time.perf_counter()
                merged = self.engine.merge_samples(allp, allv, boards=allb, canonical=self.merge_canonical, want_boards=not on_engine)
                allb, allp, allv = merged["states"] if on_engine else merged["boards"], merged["pis"], merged["zs"]
                if weighted:
                    mult = np.asarray(merged["counts"], np.uint32)
                t_merge = time.perf_counter() - t0
            perm = shuffle_permutation(allv.shape[0], seed, iteration)  # :296-297 shuffle
            allb, allp, allv = allb[perm], allp[perm], allv[perm]
            if weighted:
                mult = mult[perm]                                       # the multiplicities travel with their tuples
                samples_weight = int(mult.sum(dtype=np.uint64))
            t0 = time.perf_counter()
            if self.trainer is None:                                    # :329 -> NNet::train(samples, id, id + 1)
                self.engine.set_option("train_seed", seed + iteration)
                with self._train_optim(), self._train_validation(val_n > 0):
                    if weighted:
                        losses = self.engine.train_samples(model_id, model_id + 1, allp, allv, states=allb, weights=mult,
                                                           mirror=self.merge_canonical)
                    else:
                        losses = self.engine.train(model_id, model_id + 1, allb, allp, allv)
                    if self.validation_share > 0:
                        val_rows, val_best = self.engine.train_validation() if val_n > 0 else ([], -1)
                if self.ema_decay > 0:                                  # the candidate is the averaged model
                    self.engine.train_ema(model_id + 1)
            else:
                prev = self.engine.net_get_params(model_id)
                if weighted:
                    new = self.trainer.train(prev, allb, allp, allv, seed=seed + iteration, weights=mult, mirror=self.merge_canonical)
                else:
                    new = self.trainer.train(prev, allb, allp, allv, seed=seed + iteration)
                self.engine.net_set_params(model_id + 1, new)
                losses = list(self.trainer.history)
            t_train = time.perf_counter() - t0
            t0 = time.perf_counter()
            if rank == 0:
                self.engine.net_save(model_id + 1, os.path.join(self.dir, f"{model_id + 1}.aznet"))
            # arena: new (first listed) vs old, both seatings (:333-375); games sharded by global index across ranks,
            # the W/L/D tally is one 3-counter all-reduce
            total = 2 * (self.num_arena_games // 2)
            a_seed = seed + 7919 * (iteration + 1)
            if self.selfplay_class != -1:                               # the gate is judged in bf16 whatever the episodes were played in
                self.engine.net_set_class(model_id + 1, 0)
                self.engine.net_set_class(model_id, 0)
            with self._arena_openings():
                if world > 1 and total > 0:
                    from . import dist as azdist
                    import torch
                    import torch.distributed as tdist
                    lo, hi = azdist.shard_range(total, rank, world)
                    wld = np.zeros(3, np.uint64)
                    if hi > lo:
                        wld, _ = self.engine.arena(hi - lo, self.num_sims, new_model_id=model_id + 1, old_model_id=model_id,
                                                   seed=a_seed, max_depth=self.max_depth, cpuct=self.cpuct,
                                                   reserve=self.mcts_reserve_size, first_game=lo, total_games=total,
                                                   num_sim_threads=self.num_sim_threads)
                    dev = torch.device("cuda", torch.cuda.current_device()) if tdist.get_backend(self.group) == "nccl" else torch.device("cpu")
                    t = torch.tensor([int(x) for x in wld], dtype=torch.int64, device=dev)
                    tdist.all_reduce(t, group=self.group)
                    wld = t.cpu().numpy()
                else:
                    wld, _ = self.engine.arena(self.num_arena_games, self.num_sims, new_model_id=model_id + 1, old_model_id=model_id,
                                               seed=a_seed, max_depth=self.max_depth, cpuct=self.cpuct,
                                               reserve=self.mcts_reserve_size, num_sim_threads=self.num_sim_threads)
            t_arena = time.perf_counter() - t0
            quality, t_quality = None, None
            if self.solve_min_stones > 0:                               # the exact move-quality report of the arena just played
                t0 = time.perf_counter()
                counts = np.zeros((2, len(QUALITY_KEYS)), np.uint64)
                if world > 1 and total > 0:
                    first, local = lo, hi - lo
                else:
                    first, local = 0, total
                if local > 0:
                    game_len, moves = self.engine.arena_get_moves(local)
                    boards = self.engine.arena_get_openings(local)[0]
                    cls, _ = self.engine.move_quality(game_len, moves, start_boards=boards, max_nodes=self.solve_max_nodes,
                                                      min_stones=self.solve_min_stones)
                    counts = quality_tally(cls, first, total)
                if world > 1 and total > 0:
                    t = torch.tensor(counts.astype(np.int64).reshape(-1), dtype=torch.int64, device=dev)
                    tdist.all_reduce(t, group=self.group)
                    counts = t.cpu().numpy().reshape(2, -1)
                quality = {who: {k: int(v) for k, v in zip(QUALITY_KEYS, row)} for who, row in zip(("new", "old"), counts)}
                t_quality = time.perf_counter() - t0
                self.log(f"MOVE QUALITY (from {self.solve_min_stones} stones): NEW {quality['new']}; PREV {quality['old']}")
            nwins, pwins, draws = int(wld[0]), int(wld[1]), int(wld[2])
            self.log(f"NEW/PREV WINS : {nwins} / {pwins}; DRAWS : {draws}")            # :381
            accepted = not (pwins + nwins == 0 or nwins / (pwins + nwins) < self.update_threshold)   # :383-390
            self.log("ACCEPTING NEW MODEL" if accepted else "REJECTING NEW MODEL")
            report.append({"iteration": iteration, "samples": int(allv.shape[0]), "samples_raw": samples_raw, "nwins": nwins, "pwins": pwins,
                           "draws": draws, "accepted": accepted, "losses": losses, "model_id": model_id,
                           "seconds": {"selfplay": t_play, "train": t_train, "arena": t_arena}})
            if t_merge is not None:
                report[-1]["seconds"]["merge"] = t_merge
            if weighted:
                report[-1]["samples_weight"] = samples_weight
            if self.validation_share > 0:
                report[-1].update({"val_n": val_n, "val_loss_pi": [r[0] for r in val_rows], "val_loss_v": [r[1] for r in val_rows],
                                   "val_top1": [r[3] for r in val_rows], "best_epoch": val_best})
            if self.reanalyse_sims > 0:
                report[-1].update({"reanalysed": reanalysed, "t_reanalyse": t_reanalyse})
            if quality is not None:
                report[-1]["quality"] = quality
                report[-1]["seconds"]["quality"] = t_quality
            # a long run moves to a new model id per accepted iteration: drop the slot nobody will read again
            if free is not None:
                free(model_id if accepted else model_id + 1)
            if accepted:
                model_id += 1
            if rank == 0:
                write_state(self.dir, iteration, model_id)
            self.model_id = model_id
        return report


def reanalyse_entries(history_len):
    """csrc/az_reanalyse.h: the history entries [0, reanalyse_entries) are re-searched -- every one but the newest."""
    return history_len - 1 if history_len > 1 else 0


def reanalyse_first_game_id(iteration, history_index):
    """csrc/az_reanalyse.h: tuple j of history entry `history_index` is re-searched on game id this + j in iteration `iteration`."""
    return ((1 << 62) + (int(iteration) << 40) + (int(history_index) << 32)) & (2 ** 64 - 1)


QUALITY_KEYS = ("examined", "kept", "win_to_draw", "win_to_loss", "draw_to_loss", "unknown")


def quality_tally(ply_class, first_game, total_games):
    """The move-quality tally of one arena shard: uint64 [2, 6], row 0 the new model's moves, row 1 the old model's, columns QUALITY_KEYS.
    ply_class [n, 42] as Engine.move_quality returns it; game g of the shard has global index first_game + g.  The new model holds the
    first seat in the games below total_games // 2 (az_arena), and the first seat moves at the even plies of the record -- a start
    board, opening or not, always has the first seat to move (az_arena_get_openings)."""
    ply_class = np.asarray(ply_class)
    n = ply_class.shape[0]
    new_first = (first_game + np.arange(n)) < total_games // 2
    first_moves = np.arange(ply_class.shape[1]) % 2 == 0
    is_new = new_first[:, None] == first_moves[None, :]
    counts = np.zeros((2, len(QUALITY_KEYS)), np.uint64)
    for row, sel in ((0, is_new), (1, ~is_new)):
        k = ply_class[sel]
        counts[row, 0] = int((k != 0).sum())
        for c in range(1, len(QUALITY_KEYS)):
            counts[row, c] = int((k == c).sum())
    return counts


def write_state(directory, iteration, model_id):
    tmp = os.path.join(directory, "coach.state.tmp")
    with open(tmp, "w") as f:
        f.write(f"{int(iteration)} {int(model_id)}\n")
    os.replace(tmp, os.path.join(directory, "coach.state"))


def read_state(directory):
    """(iteration, model_id) of <dir>/coach.state, or None."""
    try:
        a, b = open(os.path.join(directory, "coach.state")).read().split()
        return int(a), int(b)
    except (OSError, ValueError):
        return None


def states_to_boards(states):
    """to_features (connect_four_game.rs:219-237, S8) for [N,2] uint64 canonical bitboards -> [N,2,6,7] f32."""
    states = np.asarray(states, np.uint64).reshape(-1, 2)
    out = np.zeros((states.shape[0], 2, 6, 7), np.float32)
    for r in range(6):
        for c in range(7):
            bit = np.uint64(1) << np.uint64(c * 7 + (5 - r))
            out[:, 0, r, c] = (states[:, 0] & bit) != 0
            out[:, 1, r, c] = (states[:, 1] & bit) != 0
    return out


def save_examples(path, history):
    """`history`: iterable of (boards [n,2,6,7], pis [n,7], vs [n]) -> "AZEX0001" file (module docstring)."""
    history = list(history)
    with open(path, "wb") as f:
        f.write(b"AZEX0001")
        np.array([len(history)] + [h[2].shape[0] for h in history], np.int64).tofile(f)
        for i in range(3):
            for h in history:
                np.ascontiguousarray(h[i], np.float32).tofile(f)


def load_examples(path):
    with open(path, "rb") as f:
        if f.read(8) != b"AZEX0001":
            raise ValueError(f"{path}: not an AZEX0001 examples file")
        H = int(np.fromfile(f, np.int64, 1)[0])
        lens = [int(x) for x in np.fromfile(f, np.int64, H)]
        boards = [np.fromfile(f, np.float32, n * 84).reshape(n, 2, 6, 7) for n in lens]
        pis = [np.fromfile(f, np.float32, n * 7).reshape(n, 7) for n in lens]
        vs = [np.fromfile(f, np.float32, n) for n in lens]
    if any(v.shape[0] != n for v, n in zip(vs, lens)):
        raise ValueError(f"{path}: truncated")
    return list(zip(boards, pis, vs))


def _mix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def shuffle_permutation(n, seed, iteration):
    """Fisher-Yates with the build's counter RNG (the reference shuffles with SmallRng, src/coach.rs:296-297; B7):
    for i = n-1 .. 1: j = ((draw(seed, iteration, i, 5) >> 32) * (i + 1)) >> 32; swap(perm[i], perm[j]).
    Same permutation as include/az_host.hpp shuffle_permutation."""
    i = np.arange(n, dtype=np.uint64)
    key = _mix64(_mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF)) ^ np.uint64(iteration))
    r = _mix64(_mix64(key ^ i) ^ np.uint64(5))
    j = ((r >> np.uint64(32)) * (i + np.uint64(1))) >> np.uint64(32)
    perm = list(range(n))
    for k in range(n - 1, 0, -1):
        t = int(j[k])
        perm[k], perm[t] = perm[t], perm[k]
    return np.array(perm, np.int64)
