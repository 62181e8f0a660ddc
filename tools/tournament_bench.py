"""One az_tournament against the K (K - 1) / 2 az_arena calls it replaces, on the same engine and models.
A warm-up of each route, then `--rounds` rounds alternating the two; the times are host clock around calls that end synchronised.
Checks that the two routes played identical games and prints leaf_rows_executed of both.
python tools/tournament_bench.py [--models 8] [--games 64] [--sims 400] [--openings 6] [--channels 512] [--rounds 3]"""
import argparse, itertools, json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np
from alphazero_rs_amd import engine as azeng

ap = argparse.ArgumentParser()
ap.add_argument("--models", type=int, default=8)
ap.add_argument("--games", type=int, default=64, help="games per pair")
ap.add_argument("--sims", type=int, default=400)
ap.add_argument("--openings", type=int, default=6)
ap.add_argument("--channels", type=int, default=512)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--seed", type=int, default=3)
a = ap.parse_args()
K, n = a.models, a.games
ids = list(range(K))
pairs = list(itertools.combinations(range(K), 2))
e = azeng.Engine(device=0, max_batch=max(4096, (K - 1) * n), net_channels=a.channels)
for k in ids:
    e.net_init_random(k, 100 + k)
e.set_arena_openings(a.openings)


def pairwise(sims, seed):
    wld = np.zeros((K, K, 3), np.uint64)
    res, moves = [], []
    for i, j in pairs:
        w, r = e.arena(n, sims, new_model_id=ids[i], old_model_id=ids[j], seed=seed)
        wld[i, j], wld[j, i] = w, (w[1], w[0], w[2])
        res.append(r.copy()); moves.append(e.arena_get_moves(n)[1])
    return wld, np.concatenate(res), np.concatenate(moves)


def timed(fn):
    e.reset_stats()
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, e.stats()["leaf_rows_executed"], out


pairwise(min(a.sims, 40), a.seed); e.tournament(ids, n, min(a.sims, 40), seed=a.seed)      # warm-up: workspaces, streams, tree arenas
t_tour, t_pair, rows = [], [], {}
for r in range(a.rounds):
    dt, rows["tournament"], got = timed(lambda: e.tournament(ids, n, a.sims, seed=a.seed))
    t_tour.append(dt)
    dt, rows["pairwise"], ref = timed(lambda: pairwise(a.sims, a.seed))
    t_pair.append(dt)
    same = np.array_equal(got["wld"], ref[0]) and np.array_equal(got["results"], ref[1]) and np.array_equal(got["moves"], ref[2])
    print(f"round {r}: tournament {t_tour[-1]:.3f} s, {len(pairs)} arenas {t_pair[-1]:.3f} s, identical games: {same}", flush=True)
    if not same:
        sys.exit("the two routes played different games")
print(json.dumps({"models": K, "games_per_pair": n, "sims": a.sims, "openings": a.openings, "channels": a.channels,
                  "tournament_s": {"median": float(np.median(t_tour)), "min": min(t_tour), "max": max(t_tour)},
                  "pairwise_s": {"median": float(np.median(t_pair)), "min": min(t_pair), "max": max(t_pair)},
                  "leaf_rows_executed": rows, "identical": True}))
