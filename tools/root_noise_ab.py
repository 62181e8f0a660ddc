"""Cost of Dirichlet root noise on the bench configuration (conv net, 8192 slots, 100 sims/move), interleaved in ONE process:
games/s and leaf_rows executed / requested per setting and round.  Noise diversifies the openings, so fewer leaves are answered by the
evaluation cache or shared inside a batch.
python tools/root_noise_ab.py [rounds=3] [episodes=16384] [slots=8192] [sims=100] [eps=0.25] [alpha=0.3]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_rs_amd import engine as azeng
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
rounds, episodes, slots, sims = arg(1, 3), arg(2, 16384), arg(3, 8192), arg(4, 100)
eps, alpha = arg(5, 0.25, float), arg(6, 0.3, float)
e = azeng.Engine(device=0, max_batch=max(slots, 256))
e.net_init_random(0, 1)
e.selfplay(n_games=256, concurrent=256, num_sims=25, model_id=0, want_boards=False)        # warm-up
for r in range(rounds):
    for x in (0.0, eps):
        e.set_root_noise(x, alpha)
        e.reset_stats()
        t = time.perf_counter()
        res = e.selfplay(n_games=episodes, concurrent=slots, num_sims=sims, model_id=0, seed=1, first_game_id=r * episodes, want_boards=False)
        dt = time.perf_counter() - t
        st = e.stats()
        print(f"round {r} eps {x:4.2f}: {episodes / dt:8.1f} games/s  plies/game {res['game_len'].mean():5.2f}  "
              f"rows executed / requested {st['leaf_rows_executed'] / max(1, st['leaf_rows_requested']):.3f}", flush=True)
e.close()
