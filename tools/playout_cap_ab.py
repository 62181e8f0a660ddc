"""Playout cap randomization ("playout_cap_sims" / "playout_cap_full_e6") at the bench configuration (conv net, C = 512, 8192 slots,
100 sims/move), interleaved in ONE process: the feature off, and cap_sims at P = 0.25 and 0.5, each in lock-step and "selfplay_async".
Per run: games/s, recorded positions/s (the tuples a trainer gets: every ply without the cap, the full plies with it) and the leaf rows
the net executed per recorded position.
python tools/playout_cap_ab.py [rounds=2] [episodes=16384] [slots=8192] [sims=100] [cap_sims=20] [channels=512]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_rs_amd import engine as azeng
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
rounds, episodes, slots, sims, cap_sims, channels = arg(1, 2), arg(2, 16384), arg(3, 8192), arg(4, 100), arg(5, 20), arg(6, 512)
e = azeng.Engine(device=0, max_batch=max(slots, 256), net_channels=channels)
e.net_init_random(0, 1)
e.selfplay(n_games=256, concurrent=256, num_sims=25, model_id=0, want_boards=False)        # warm-up
for r in range(rounds):
    for async_mode in (0, 1):
        for n, p in ((0, 0.25), (cap_sims, 0.25), (cap_sims, 0.5)):
            e.set_option("selfplay_async", async_mode)
            e.set_playout_cap(n, p)
            e.reset_stats()
            t = time.perf_counter()
            res = e.selfplay(n_games=episodes, concurrent=slots, num_sims=sims, model_id=0, seed=1, first_game_id=r * episodes,
                             symmetries=False, want_boards=False)
            dt = time.perf_counter() - t
            st = e.stats()
            print(f"round {r} {'async    ' if async_mode else 'lock-step'} cap {n:3d} P {p:4.2f}: {episodes / dt:8.1f} games/s  "
                  f"{res['count'] / dt:10.1f} recorded positions/s  plies/game {res['game_len'].mean():5.2f}  "
                  f"sims/ply {st['simulations'] / max(1, st['moves']):6.2f}  "
                  f"executed leaf rows / recorded position {st['leaf_rows_executed'] / max(1, res['count']):7.2f}", flush=True)
e.set_playout_cap(0)
e.set_option("selfplay_async", 0)
e.close()
