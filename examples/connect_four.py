#!/usr/bin/env python3
"""The reference's example binary (examples/connect_four.rs:53-77) on the MI355X engine: the same 15 Coach::setup
literals by default (25 sims, 1 episode, 40 arena games, stub net when --net stub), or a real run with the bf16
conv net (--net conv) and bigger numbers.  Needs a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from alphazero_rs_amd import engine as azeng            # noqa: E402
from alphazero_rs_amd.coach import Coach                # noqa: E402
from alphazero_rs_amd.trainer import Trainer            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default="./checkpoint")
    ap.add_argument("--net", default="conv", choices=["conv"])
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--iters", type=int, default=1)          # num_iters, examples/connect_four.rs:65
    ap.add_argument("--eps", type=int, default=1)            # num_eps, :66
    ap.add_argument("--sims", type=int, default=25)          # num_sims, :67
    ap.add_argument("--arena", type=int, default=40)         # num_arena_games, :64
    ap.add_argument("--slots", type=int, default=8192)       # concurrent games (num_episode_threads, :63)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--trainer", default="engine", choices=["engine", "torch"])   # NNet::train: az_net_train or autograd
    ap.add_argument("--epochs", type=int, default=10)        # connect_four_net.py:13
    ap.add_argument("--selfplay-fp8", action="store_true")   # episodes in the fp8 class, the arena gate in bf16 (Coach.selfplay_class)
    ap.add_argument("--playout-cap", default=None, metavar="N,P")        # playout cap randomization of the episodes, e.g. 20,0.25 (Coach.playout_cap_sims)
    ap.add_argument("--forced-playouts", default=None, metavar="K[,prune]")   # forced playouts at the root, e.g. 2,prune: with policy target pruning (Coach.forced_playouts_k)
    ap.add_argument("--gumbel", default=None, metavar="M[,CVISIT,CSCALE]")   # Gumbel root search with sequential halving in the episodes, e.g. 4 or 4,50,1: at most M root actions considered (Coach.gumbel_m)
    ap.add_argument("--arena-openings", type=int, default=0, metavar="N")   # paired openings of the gate: N random quiet plies (even, 2 .. 12) per pair of arena games (Coach.arena_opening_plies)
    ap.add_argument("--weight-decay", type=float, default=0.0)       # decoupled AdamW decay of the weight tensors in NNet::train, e.g. 1e-4 (Coach.weight_decay)
    ap.add_argument("--clip-norm", type=float, default=0.0)          # global gradient-norm clipping, e.g. 1.0 (Coach.clip_norm)
    ap.add_argument("--lr-schedule", default=None, metavar="WARMUP,MODE,FLOOR")   # e.g. 100,cosine,0.1: linear warm-up over WARMUP steps, then cosine / linear / none down to FLOOR x lr over the call's steps (Coach.lr_warmup_steps / lr_decay / lr_floor)
    ap.add_argument("--ema", type=float, default=0.0)                # decay of the averaged weights, e.g. 0.999: the candidate is the averaged model (Coach.ema_decay)
    ap.add_argument("--merge-positions", nargs="?", const="plain", default=None, choices=["plain", "canonical", "weighted", "canonical,weighted"])   # position averaging before training: one tuple per distinct position; canonical also merges mirror images (Coach.merge_positions); weighted draws every training row in proportion to its multiplicity (Coach.merge_weighted)
    ap.add_argument("--move-quality", default=None, metavar="STONES[,NODES]")   # exact move-quality report of every arena: positions with at least STONES stones are solved (budget NODES per position and action, default 2^20) and each model's value-losing moves counted (Coach.solve_min_stones)
    ap.add_argument("--value-target-q", type=float, default=0.0, metavar="L")   # value target (1 - L) z + L q: the game outcome mixed with the root value of the tuple's own search, e.g. 0.5 (Coach.value_target_q)
    ap.add_argument("--surprise", type=float, default=0.0, metavar="S")   # policy surprise weighting: the iteration's tuples resampled, a share S of the weight in proportion to KL(pi || root prior), e.g. 0.5 (Coach.surprise_share)
    ap.add_argument("--validation", default=None, metavar="SHARE[,PATIENCE[,best]]")   # held-out validation, e.g. 0.05 or 0.05,3,best: a share SHARE of the window's positions is never trained on and scored at the end of every epoch; PATIENCE > 0 stops after that many epochs without a new best, best keeps the best epoch's weights (Coach.validation_share / patience / keep_best)
    ap.add_argument("--reanalyse", type=int, default=0, metavar="SIMS")   # every iteration the pi of every tuple of the older history windows is replaced by a fresh search of SIMS simulations with the current net, before the window is saved and trained on, e.g. 50 (Coach.reanalyse_sims)
    ap.add_argument("--root-noise", default=None, metavar="EPS,ALPHA")   # Dirichlet root noise of the episodes, e.g. 0.25,0.3 (Coach.root_noise_eps)
    ap.add_argument("--eval-mirror", action="store_true")    # mirror-canonical leaf evaluation for the whole loop (Coach.eval_mirror)
    ap.add_argument("--search-stop", action="store_true")    # the decided-move stop for the whole loop: a temperature-0 search of the episodes and every search of the gate ends once its move can no longer change (Coach.search_stop)
    a = ap.parse_args()
    e = azeng.Engine(device=0, max_batch=max(a.slots, a.arena, 128), net_channels=a.channels)
    e.net_init_random(0, a.seed)
    e.set_option("train_epochs", a.epochs)
    coach = Coach.setup(e, a.checkpoint,
                        1000000,   # mcts_reserve_size
                        0.6,       # update_threshold
                        15,        # temp_threshold
                        20,        # max_history_length
                        200000,    # max_queue_length
                        1,         # inference_batch_size
                        a.slots,   # num_episode_threads -> concurrent game slots
                        a.arena,   # num_arena_games
                        a.iters,   # num_iters
                        a.eps,     # num_eps
                        a.sims,    # num_sims
                        1,         # num_sim_threads
                        1000,      # max_depth
                        1,         # cpuct
                        trainer=Trainer(channels=a.channels, epochs=a.epochs) if a.trainer == "torch" else None)
    if a.selfplay_fp8:
        coach.selfplay_class = azeng.NET_CLASS_FP8
    coach.eval_mirror = a.eval_mirror
    coach.search_stop = a.search_stop
    if a.root_noise:
        eps, _, alpha = a.root_noise.partition(",")
        coach.root_noise_eps, coach.root_noise_alpha = float(eps), float(alpha) if alpha else 1.0
    if a.playout_cap:
        n, _, p = a.playout_cap.partition(",")
        coach.playout_cap_sims, coach.playout_cap_full = int(n), float(p) if p else 0.25
    if a.forced_playouts:
        k, _, prune = a.forced_playouts.partition(",")
        coach.forced_playouts_k, coach.policy_prune = float(k), prune == "prune"
    if a.gumbel:
        parts = a.gumbel.split(",")
        coach.gumbel_m = int(parts[0])
        coach.gumbel_c_visit, coach.gumbel_c_scale = (float(parts[1]) if len(parts) > 1 else 50.0), (float(parts[2]) if len(parts) > 2 else 1.0)
    coach.arena_opening_plies = a.arena_openings
    coach.value_target_q, coach.surprise_share = a.value_target_q, a.surprise
    coach.reanalyse_sims = a.reanalyse
    coach.weight_decay, coach.clip_norm, coach.ema_decay = a.weight_decay, a.clip_norm, a.ema
    if a.lr_schedule:
        parts = a.lr_schedule.split(",")
        coach.lr_warmup_steps = int(parts[0])
        mode = parts[1] if len(parts) > 1 else "none"
        coach.lr_decay = {"none": 0, "cosine": 1, "linear": 2}[mode] if mode in ("none", "cosine", "linear") else int(mode)
        coach.lr_floor = float(parts[2]) if len(parts) > 2 else 0.0
    modes = (a.merge_positions or "").split(",")
    coach.merge_positions, coach.merge_canonical, coach.merge_weighted = a.merge_positions is not None, "canonical" in modes, "weighted" in modes
    if a.validation:
        parts = a.validation.split(",")
        coach.validation_share = float(parts[0])
        coach.patience = int(parts[1]) if len(parts) > 1 and parts[1] else 0
        coach.keep_best = len(parts) > 2 and parts[2] == "best"
    if a.move_quality:
        stones, _, nodes = a.move_quality.partition(",")
        coach.solve_min_stones, coach.solve_max_nodes = int(stones), int(nodes) if nodes else 1 << 20
    for r in coach.learn(skip_first_play=False, seed=a.seed):
        print(r["iteration"], "samples", r["samples"], *(("of", r["samples_raw"]) if coach.merge_positions else ()), "new/prev/draw", r["nwins"], r["pwins"], r["draws"],
              "accepted" if r["accepted"] else "rejected", "loss", r["losses"][-1],
              "seconds", {k: round(v, 2) for k, v in r["seconds"].items()})
        if "val_n" in r:
            print(r["iteration"], "held out", r["val_n"], "val loss_pi", [round(x, 4) for x in r["val_loss_pi"]], "loss_v", [round(x, 4) for x in r["val_loss_v"]],
                  "top1", [round(x, 4) for x in r["val_top1"]], "best epoch", r["best_epoch"])
        if "reanalysed" in r:
            print(r["iteration"], "older tuples re-searched", r["reanalysed"], "in", round(r["t_reanalyse"], 2), "s")
        if "quality" in r:
            print(r["iteration"], "move quality from", coach.solve_min_stones, "stones:", r["quality"])
    e.close()


if __name__ == "__main__":
    main()
