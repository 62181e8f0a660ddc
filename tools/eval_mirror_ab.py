"""The opt-in "eval_mirror" (mirror-canonical leaf evaluation) against the default at the bench configuration (conv net, C = 512, 65536
episodes on 8192 slots, 100 sims/move), alternating in ONE process: per run games/s, leaf rows executed / requested, cache hits and batch
duplicates.  A position and its mirror image share one batch row and one evaluation-cache entry with the option on, so the net runs on
fewer rows; the games differ (F is another function than the raw net), the work per game does not.
python tools/eval_mirror_ab.py [rounds=3] [episodes=65536] [slots=8192] [sims=100] [channels=512]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_rs_amd import engine as azeng
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
rounds, episodes, slots, sims, channels = arg(1, 3), arg(2, 65536), arg(3, 8192), arg(4, 100), arg(5, 512)
e = azeng.Engine(device=0, max_batch=max(slots, 256), net_channels=channels)
e.net_init_random(0, 1)
e.selfplay(n_games=256, concurrent=256, num_sims=25, model_id=0, want_boards=False)        # warm-up
for r in range(rounds):
    for on in (0, 1):
        e.set_eval_mirror(on)
        e.reset_stats()
        t = time.perf_counter()
        res = e.selfplay(n_games=episodes, concurrent=slots, num_sims=sims, model_id=0, seed=1, first_game_id=r * episodes, want_boards=False)
        dt = time.perf_counter() - t
        st = e.stats()
        req = max(1, st["leaf_rows_requested"])
        print(f"round {r} eval_mirror {on}: {episodes / dt:8.1f} games/s  plies/game {res['game_len'].mean():5.2f}  "
              f"rows executed / requested {st['leaf_rows_executed'] / req:.3f} ({st['leaf_rows_executed']} / {st['leaf_rows_requested']})  "
              f"cache hits {st['eval_cache_hits'] / req:.3f}  batch dups {st['eval_batch_dups'] / req:.3f}", flush=True)
e.set_eval_mirror(0)
e.close()
