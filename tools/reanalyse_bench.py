"""az_reanalyse (include/az_reanalyse.h) on one GPU with a randomly initialised conv net.  A measurement, no
pass/fail bar.
The window is the tuples of one self-play of `episodes` episodes at `sims` simulations (no symmetries), cut to `window` positions when that
is given.  Measured, in bf16 and in fp8, with a cold cache (cleared by every call) and a warm one ("eval_cache_persist", filled by a call
that is not counted): az_reanalyse at `concurrent` trees, against the route there was before it for identical results -- a host loop of
az_tree_reset + az_tree_get_action_prob over chunks of `concurrent` trees, host arrays in and out (the last chunk padded).  `rounds`
alternating rounds; best, and the spread over the rounds.  The two routes' pi, counts and q are compared once per class (they must be equal).
python tools/reanalyse_bench.py [episodes=8192] [sims=100] [concurrent=8192] [channels=512] [rounds=3] [window=0] [cache_log2=28]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (before the engine library is loaded: a process wants one HIP runtime)
from alphazero_rs_amd import engine as azeng
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
episodes, sims, concurrent, channels, rounds, window, cache_log2 = arg(1, 8192), arg(2, 100), arg(3, 8192), arg(4, 512), arg(5, 3), arg(6, 0), arg(7, 28)
SEED, FIRST, RESERVE = 1, 1 << 40, 1000000

e = azeng.Engine(device=0, max_batch=max(concurrent, min(episodes, 8192)), net_channels=channels)
e.net_init_random(0, SEED)
t = time.perf_counter()
e.reset_stats()
res = e.selfplay(n_games=episodes, concurrent=min(episodes, 8192), num_sims=sims, model_id=0, seed=SEED, symmetries=False, want_boards=False)
dt = time.perf_counter() - t
n = res["count"] if window <= 0 else min(window, res["count"])
states = np.ascontiguousarray(res["states"][:n])
print(f"window: {n} of the {res['count']} tuples of {episodes} episodes x {sims} simulations; that self-play (first call, arenas allocated): "
      f"{dt:.2f} s, {e.stats()['simulations'] / dt:.0f} simulations/s", flush=True)


def by_reanalyse():
    return e.reanalyse(sims, 0, states=states, seed=SEED, first_game_id=FIRST, concurrent=concurrent, reserve=RESERVE,
                       out={"root_q": None, "root_prior": None, "selected": None})


tb = None


def by_host_loop():
    """What the engine offered before: one tree batch, re-rooted and searched chunk by chunk."""
    pi, counts, q = np.zeros((n, 7), np.float32), np.zeros((n, 7), np.uint16), np.zeros((n, 7), np.float32)
    for off in range(0, n, concurrent):
        k = min(concurrent, n - off)
        chunk = states[off:off + k]
        if k < concurrent:
            chunk = np.concatenate([chunk, np.repeat(states[:1], concurrent - k, axis=0)])
        tb.reset(chunk)
        p, c, qq = tb.get_action_prob(chunk, 1.0, seed=SEED, first_game_id=FIRST + off)
        pi[off:off + k], counts[off:off + k], q[off:off + k] = p[:k], c[:k], qq[:k]
    return {"pi": pi, "counts": counts, "q": q}


def timed(fn):
    e.reset_stats()
    t = time.perf_counter()
    got = fn()
    return time.perf_counter() - t, got, e.stats()


for name, klass in (("bf16", azeng.NET_CLASS_BF16), ("fp8", azeng.NET_CLASS_FP8)):
    e.net_set_class(0, klass)
    for cache in ("cold", "warm"):
        e.set_option("eval_cache_log2", cache_log2 if cache == "warm" else 30)
        e.set_option("eval_cache_persist", 1 if cache == "warm" else 0)
        tb = e.tree_create(concurrent, reserve=RESERVE, num_sims=sims, max_depth=1000, model_id=0, cpuct=1)
        a, b = by_reanalyse(), by_host_loop()                         # arenas, workspaces, graphs -- and the warm cache's content; not counted
        same = all(np.array_equal(a[k], b[k]) for k in ("pi", "counts", "q"))
        times = {"az_reanalyse": [], "host loop": []}
        rows = {}
        for r in range(rounds):
            for route, fn in (("az_reanalyse", by_reanalyse), ("host loop", by_host_loop)):
                dt, _, st = timed(fn)
                times[route].append(dt)
                rows[route] = (st["leaf_rows_requested"], st["leaf_rows_executed"], st["simulations"])
        tb.close()
        for route, ts in times.items():
            best = min(ts)
            nsim = n * sims
            print(f"{name} {cache} cache, {route:12s}: best of {rounds} {best:8.3f} s (spread {max(ts) - best:.3f} s), {n / best:10.0f} positions/s, "
                  f"{nsim / best:12.0f} simulations/s; leaf rows requested {rows[route][0]} executed {rows[route][1]}", flush=True)
        print(f"{name} {cache} cache: az_reanalyse is {min(times['host loop']) / min(times['az_reanalyse']):.2f} x the host loop; results "
              f"{'identical' if same else 'DIFFER'}", flush=True)
e.set_option("eval_cache_persist", 0)
e.set_option("eval_cache_log2", 30)
e.net_set_class(0, azeng.NET_CLASS_ENGINE)
e.close()
