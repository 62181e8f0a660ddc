"""Search statistics as training targets (Coach.value_target_q / Coach.surprise_share; csrc/az_target.h) on one GPU from
one seed with a randomly initialised conv net.  A measurement, no pass/fail bar.
Part 1 (mode "cost" or "all"): az_selfplay wall time with "selfplay_record_search" on against off in alternating rounds -- the cost of the
record kernel and the second emit --, then az_samples_blend_z and az_samples_surprise on a window of `window` tuples by the states and the
boards routes.
Part 2 (mode "loops" or "all"): two Coach loops of the same iterations and episodes that differ in ONE option -- `option` = value_target_q or
surprise_share at `value`, against the plain loop -- each into its own directory under `out`, which is kept: tools/rate_checkpoints.py rates
the <id>.aznet files of the two directories against each other.  Playing strength is whatever that rating says; this tool prints only the
per-iteration sample counts, gate scores and times.
python tools/search_targets_ab.py [mode=all] [option=value_target_q] [value=0.5] [iters=3] [episodes=4096] [slots=8192] [sims=100] [channels=512]
                                  [arena=256] [epochs=1] [rounds=3] [window=372000] [out=./search_targets_ab]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from alphazero_rs_amd import engine as azeng
from alphazero_rs_amd.coach import Coach, states_to_boards
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
mode, option, value = arg(1, "all", str), arg(2, "value_target_q", str), arg(3, 0.5, float)
iters, episodes, slots, sims, channels, arena, epochs, rounds, window = (arg(4, 3), arg(5, 4096), arg(6, 8192), arg(7, 100), arg(8, 512), arg(9, 256),
                                                                         arg(10, 1), arg(11, 3), arg(12, 372000))
out = arg(13, "./search_targets_ab", str)
SEED = 1
if option not in ("value_target_q", "surprise_share"):
    sys.exit("option must be value_target_q or surprise_share")

if mode in ("cost", "all"):
    e = azeng.Engine(device=0, max_batch=max(slots, arena, 256), net_channels=channels)
    e.net_init_random(0, SEED)
    e.selfplay(n_games=256, concurrent=256, num_sims=25, model_id=0, want_boards=False)        # warm-up
    n_tp = max(episodes, slots)
    times = {0: [], 1: []}
    last = None
    for r in range(rounds):
        for on in (0, 1):
            e.set_option("selfplay_record_search", on)
            t = time.perf_counter()
            res = e.selfplay(n_games=n_tp, concurrent=slots, num_sims=sims, model_id=0, seed=SEED, first_game_id=0, symmetries=False, want_boards=False)
            dt = time.perf_counter() - t
            times[on].append(dt)
            print(f"self-play round {r} record_search {on}: {dt:7.3f} s  {n_tp / dt:8.1f} games/s  tuples {res['count']}", flush=True)
            if on:
                last = (res, e.selfplay_search())
    e.set_option("selfplay_record_search", 0)
    off, on = min(times[0]), min(times[1])
    print(f"self-play {n_tp} episodes, {slots} slots, {sims} simulations: best of {rounds} off {off:.3f} s, on {on:.3f} s ({100.0 * (on - off) / off:+.2f} %); "
          f"spread off {max(times[0]) - off:.3f} s, on {max(times[1]) - on:.3f} s")
    # the consumers on a window of `window` tuples: the recorded tuples, repeated
    res, (rq, rp) = last
    idx = np.arange(window) % res["count"]
    states, pis, zs, rq, rp = res["states"][idx], res["pis"][idx], res["zs"][idx], rq[idx], rp[idx]
    boards = states_to_boards(states)
    for name, fn in (("blend_z", lambda: e.blend_z(zs, rq, 0.5)),
                     ("surprise states", lambda: e.surprise(pis, zs, rp, 0.5, SEED, states=states)),
                     ("surprise boards", lambda: e.surprise(pis, zs, rp, 0.5, SEED, boards=boards)),
                     ("surprise counts only", lambda: e.surprise(pis, zs, rp, 0.5, SEED, states=states, want=False))):
        best_wall, best_dev = 1e30, 1e30
        for r in range(rounds + 1):                               # the first call sizes the workspace
            e.reset_stats()
            t = time.perf_counter()
            got = fn()
            best_wall = min(best_wall, time.perf_counter() - t)
            best_dev = min(best_dev, e.stats()["device_ms"])
        extra = f"  rows out {got['count']}, mean KL {float(got['kl'].mean()):.4f}, largest c_i {int(got['counts'].max())}" if isinstance(got, dict) and "count" in got else ""
        print(f"{name} on {window} tuples: call {1e3 * best_wall:8.2f} ms wall (host arrays in and out), {best_dev:8.2f} ms inside the engine{extra}", flush=True)
    e.close()

if mode in ("loops", "all"):
    table = []
    for name, v in (("plain", 0.0), (f"{option}-{value:g}", value)):
        d = os.path.join(out, name)
        os.makedirs(d, exist_ok=True)
        e = azeng.Engine(device=0, max_batch=max(slots, arena, 256), net_channels=channels)
        try:
            e.net_init_random(0, SEED)
            e.set_option("train_epochs", epochs)
            coach = Coach.setup(e, d, 1000000, 0.55, 15, 20, 200000, 1, slots, arena, iters, episodes, sims, 1, 1000, 1, log=lambda s: None)
            setattr(coach, option, v)
            for rep in coach.learn(skip_first_play=False, seed=SEED):
                s = rep["seconds"]
                print(f"{name} iteration {rep['iteration']}: samples {rep['samples']}  gate new/prev/draw {rep['nwins']}/{rep['pwins']}/{rep['draws']} "
                      f"{'accepted' if rep['accepted'] else 'rejected'}  self-play {s['selfplay']:.2f} s  train {s['train']:.2f} s", flush=True)
                table.append((name, rep["iteration"], rep["samples"], rep["nwins"], rep["pwins"], rep["draws"], rep["accepted"], s["selfplay"]))
        finally:
            e.close()
    print("\n| loop | iteration | samples | gate new/prev/draw | accepted | self-play s |\n|---|---|---|---|---|---|")
    for name, it, n, nw, pw, dr, acc, sp in table:
        print(f"| {name} | {it} | {n} | {nw}/{pw}/{dr} | {'yes' if acc else 'no'} | {sp:.2f} |")
    print(f"\ncheckpoints kept under {out}/: rate them with tools/rate_checkpoints.py")
