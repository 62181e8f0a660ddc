"""Forced playouts with policy target pruning ("forced_playouts_k_e6" / "policy_prune") against the default at the bench configuration
(conv net, C = 512, 8192 slots, 100 sims/move) with Dirichlet root noise 0.25 on in both, interleaved in ONE process.  Per run: games/s,
leaf rows executed / requested (forced playouts diversify the searches, so the cache answers fewer leaves), the mean entropy of the
recorded pi (nats) and the mean share of visits pruned.  The self-play entries return pi but not the raw counts, so the pruned share is
measured on az_tree_get_action_prob searches (fresh trees, the same sims, temperature 1) of `probe` positions recorded by the run: there
counts are raw, pi = m / sum(m) and the most visited child keeps its count, so sum(m) = counts[b] / pi[b].
python tools/forced_playouts_ab.py [rounds=2] [episodes=16384] [slots=8192] [sims=100] [k=2.0] [channels=512] [probe=4096]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_rs_amd import engine as azeng
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
rounds, episodes, slots, sims, k_on, channels, probe = arg(1, 2), arg(2, 16384), arg(3, 8192), arg(4, 100), arg(5, 2.0, float), arg(6, 512), arg(7, 4096)
e = azeng.Engine(device=0, max_batch=max(slots, 256), net_channels=channels)
e.net_init_random(0, 1)
e.selfplay(n_games=256, concurrent=256, num_sims=25, model_id=0, want_boards=False)        # warm-up
e.set_root_noise(0.25, 0.3)
for r in range(rounds):
    for k in (0.0, k_on):
        e.set_forced_playouts(k, prune=k > 0)
        e.reset_stats()
        t = time.perf_counter()
        res = e.selfplay(n_games=episodes, concurrent=slots, num_sims=sims, model_id=0, seed=1, first_game_id=r * episodes, symmetries=False,
                         want_boards=False)
        dt = time.perf_counter() - t
        st = e.stats()
        req = max(1, st["leaf_rows_requested"])
        pi = res["pis"].astype(np.float64)
        ent = -(pi * np.log(np.where(pi > 0, pi, 1.0))).sum(axis=1).mean()
        # the pruned share, on fresh searches of recorded positions (every (count // probe)-th tuple)
        states = res["states"][:: max(1, res["count"] // probe)][:probe]
        tb = e.tree_create(len(states), reserve=8 * sims + 64, num_sims=sims, max_depth=1000, model_id=0, cpuct=1)
        tpi, counts, _ = tb.get_action_prob(states, 1.0, seed=1, first_game_id=r * episodes)
        tb.close()
        b = counts.shape[1] - 1 - counts[:, ::-1].argmax(axis=1)       # the most visited child, the highest among equals: it keeps its count
        rows = np.arange(len(states))
        kept = counts[rows, b] / np.maximum(tpi[rows, b].astype(np.float64), 1e-30)
        pruned = 1.0 - kept / np.maximum(1, counts.sum(axis=1))
        print(f"round {r} k {k:3.1f} prune {int(k > 0)}: {episodes / dt:8.1f} games/s  plies/game {res['game_len'].mean():5.2f}  "
              f"rows executed / requested {st['leaf_rows_executed'] / req:.3f} ({st['leaf_rows_executed']} / {st['leaf_rows_requested']})  "
              f"pi entropy {ent:.3f}  visits pruned {max(0.0, pruned.mean()):.3f} (on {len(states)} recorded positions)", flush=True)
e.set_forced_playouts(0.0)
e.set_root_noise(0.0, 1.0)
e.close()
