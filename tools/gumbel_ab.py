"""Gumbel root search ("gumbel_m") against PUCT, on one GPU from one seed with a randomly initialised conv net.  A measurement, no pass/fail bar.
Part 1, throughput: az_selfplay games/s with gumbel_m = `m` and with PUCT at 16 and at 100 simulations per move, `slots` concurrent games,
interleaved in ONE process.  Part 2, three short Coach loops of the same iterations and episodes -- Gumbel at 16 simulations, PUCT at 16,
PUCT at 100 --: per iteration the self-play games/s, the exact move-quality tally of the arena's games from `stones` stones on
(az_move_quality: value-losing moves of the NEW model) and the gate's score.  Prints one line per measurement and a markdown table at the end.
python tools/gumbel_ab.py [iters=3] [episodes=4096] [slots=8192] [channels=512] [arena=256] [stones=26] [epochs=1] [m=4] [rounds=2]"""
import os, shutil, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_rs_amd import engine as azeng
from alphazero_rs_amd.coach import Coach
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
iters, episodes, slots, channels, arena, stones, epochs, m, rounds = (arg(1, 3), arg(2, 4096), arg(3, 8192), arg(4, 512), arg(5, 256), arg(6, 26),
                                                                       arg(7, 1), arg(8, 4), arg(9, 2))
SEED = 1
rows = []

# ---- part 1: self-play throughput at the same budgets and shapes --------------------------------------------------------------------------
e = azeng.Engine(device=0, max_batch=max(slots, arena, 256), net_channels=channels)
e.net_init_random(0, SEED)
e.selfplay(n_games=256, concurrent=256, num_sims=25, model_id=0, want_boards=False)        # warm-up
n_tp = max(episodes, slots)
for r in range(rounds):
    for sims in (16, 100):
        for gm in (0, m):
            e.set_gumbel(gm)
            e.reset_stats()
            t = time.perf_counter()
            res = e.selfplay(n_games=n_tp, concurrent=slots, num_sims=sims, model_id=0, seed=SEED, first_game_id=r * n_tp, symmetries=False, want_boards=False)
            dt = time.perf_counter() - t
            st = e.stats()
            print(f"throughput round {r} sims {sims:3d} {'gumbel m=%d' % gm if gm else 'puct      '}: {n_tp / dt:8.1f} games/s  plies/game {res['game_len'].mean():5.2f}  "
                  f"rows executed / requested {st['leaf_rows_executed'] / max(1, st['leaf_rows_requested']):.3f}", flush=True)
            rows.append(("throughput", r, "gumbel" if gm else "puct", sims, n_tp / dt))
e.set_gumbel(0)
e.close()

# ---- part 2: three Coach loops ------------------------------------------------------------------------------------------------------------
table = []
for name, gm, sims in (("gumbel-16", m, 16), ("puct-16", 0, 16), ("puct-100", 0, 100)):
    d = tempfile.mkdtemp(prefix="gumbel_ab_")
    e = azeng.Engine(device=0, max_batch=max(slots, arena, 256), net_channels=channels)
    try:
        e.net_init_random(0, SEED)
        e.set_option("train_epochs", epochs)
        coach = Coach.setup(e, d, 1000000, 0.55, 15, 20, 200000, 1, slots, arena, iters, episodes, sims, 1, 1000, 1, log=lambda s: None)
        coach.gumbel_m = gm
        coach.solve_min_stones = stones
        for rep in coach.learn(skip_first_play=False, seed=SEED):
            q = rep["quality"]["new"]
            lost = q["win_to_draw"] + q["win_to_loss"] + q["draw_to_loss"]
            gps = episodes / rep["seconds"]["selfplay"]
            print(f"{name} iteration {rep['iteration']}: {gps:8.1f} self-play games/s  samples {rep['samples']}  move quality (new model, from {stones} stones) "
                  f"{q}  gate new/prev/draw {rep['nwins']}/{rep['pwins']}/{rep['draws']} {'accepted' if rep['accepted'] else 'rejected'}", flush=True)
            table.append((name, rep["iteration"], gps, q["examined"], lost, q["unknown"], rep["nwins"], rep["pwins"], rep["draws"], rep["accepted"]))
    finally:
        e.close()
        shutil.rmtree(d, ignore_errors=True)

print("\n| sims | PUCT games/s | Gumbel m=%d games/s |\n|---|---|---|" % m)
for sims in (16, 100):
    best = {k: max(v for kind, _, k2, s, v in rows if k2 == k and s == sims) for k in ("puct", "gumbel")}
    print(f"| {sims} | {best['puct']:.0f} | {best['gumbel']:.0f} |")
print("\n| loop | iteration | self-play games/s | moves examined | value-losing | unknown | gate new/prev/draw | accepted |\n|---|---|---|---|---|---|---|---|")
for name, it, gps, ex, lost, unk, nw, pw, dr, acc in table:
    print(f"| {name} | {it} | {gps:.0f} | {ex} | {lost} ({100.0 * lost / max(1, ex):.1f} %) | {unk} | {nw}/{pw}/{dr} | {'yes' if acc else 'no'} |")
