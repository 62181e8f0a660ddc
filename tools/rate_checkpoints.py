"""Rate the checkpoints of one or more Coach directories in one pool: one az_tournament with paired openings, then az_rating_fit.
The instrument for the README's "playing strength unmeasured" rows: run two loops that differ in one option, then rate both directories'
checkpoints together.
python tools/rate_checkpoints.py DIR[:label] [DIR[:label] ...] [--games 64] [--sims 100] [--openings 6] [--every 1] [--last 0] [--max 16]
                                 [--channels 512] [--seed 0] [--prior 2.0]"""
import argparse, os, re, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
from alphazero_rs_amd import engine as azeng

ap = argparse.ArgumentParser()
ap.add_argument("dirs", nargs="+", metavar="DIR[:label]")
ap.add_argument("--games", type=int, default=64, help="games per pair (even)")
ap.add_argument("--sims", type=int, default=100)
ap.add_argument("--openings", type=int, default=6, help="random opening plies per game pair (even, 0 = off)")
ap.add_argument("--every", type=int, default=1, help="take every n-th checkpoint of a directory")
ap.add_argument("--last", type=int, default=0, help="only the last n checkpoints of a directory (0 = all)")
ap.add_argument("--max", type=int, default=16, help="cap on the pool (at most 16): the newest checkpoints of each directory are kept")
ap.add_argument("--channels", type=int, default=512)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--prior", type=float, default=2.0)
a = ap.parse_args()
if not 2 <= a.max <= 16:
    sys.exit("--max must be in 2 .. 16")
per_dir = []
for spec in a.dirs:
    d, _, label = spec.partition(":")
    label = label or os.path.basename(os.path.normpath(d))
    nums = sorted(int(m.group(1)) for m in (re.fullmatch(r"(\d+)\.aznet", f) for f in os.listdir(d)) if m)
    nums = nums[::-1][::max(1, a.every)][::-1]            # every n-th, counted from the newest
    if a.last > 0:
        nums = nums[-a.last:]
    per_dir.append([(f"{label}/{k}", os.path.join(d, f"{k}.aznet")) for k in nums])
share = max(1, a.max // len(per_dir))
pool = [x for lst in per_dir for x in lst[-share:]][:a.max]
if len(pool) < 2:
    sys.exit("fewer than two checkpoints found")
K = len(pool)
e = azeng.Engine(device=0, max_batch=max(4096, (K - 1) * a.games), net_channels=a.channels)
for k, (_, path) in enumerate(pool):
    e.net_load(k, path)
e.set_arena_openings(a.openings)
got = e.tournament(list(range(K)), a.games, a.sims, seed=a.seed)
elo, se, sweeps = azeng.rating_fit(got["wld"], a.prior)
names = [n for n, _ in pool]
w = max(len(n) for n in names)
print(f"{K} checkpoints, {a.games} games per pair ({len(got['results'])} games), {a.sims} simulations, openings {a.openings}, seed {a.seed}")
print("W/L/D, row against column:")
for i in range(K):
    print(f"{names[i]:>{w}} " + " ".join("      -    " if i == j else "%3d/%3d/%3d" % tuple(int(x) for x in got["wld"][i, j]) for j in range(K)))
print(f"Elo (mean 0, prior {a.prior} games per pair, {sweeps} sweeps; elo_se is the diagonal Fisher approximation):")
for i in sorted(range(K), key=lambda i: -elo[i]):
    print(f"{names[i]:>{w}} {elo[i]:+8.1f} +- {se[i]:.1f}")
