"""Paired arena openings ("arena_opening_plies") off and on: how many DIFFERENT games an arena of a conv model against itself holds.  The
arena searches at temperature 0 and a conv net is a function of the state, so from one position every game of a seating is the same game
apart from count ties; with openings every pair starts elsewhere.  Prints, per setting, the number of distinct (opening, moves) records,
the W/L/D tally and games/s (the two rates are not like for like: games from openings are shorter and hit the cache differently).
python tools/arena_openings_ab.py [games=64] [sims=50] [plies=6] [channels=512]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_rs_amd import engine as azeng
arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
games, sims, plies, channels = arg(1, 64), arg(2, 50), arg(3, 6), arg(4, 512)
e = azeng.Engine(device=0, max_batch=max(games, 256), net_channels=channels)
e.net_init_random(0, 1)
e.arena(16, 25, new_model_id=0, old_model_id=0)        # warm-up
for n in (0, plies):
    e.set_arena_openings(n)
    t = time.perf_counter()
    wld, res = e.arena(games, sims, new_model_id=0, old_model_id=0, seed=3)
    dt = time.perf_counter() - t
    boards, _, _ = e.arena_get_openings(len(res))
    glen, moves = e.arena_get_moves(len(res))
    distinct = len({(tuple(boards[g].tolist()), tuple(moves[g, :glen[g]].tolist())) for g in range(len(res))})
    print(f"arena_opening_plies = {n}: {distinct} distinct games of {len(res)}, W/L/D {wld.tolist()}, mean length {glen.mean():.1f} plies, {len(res) / dt:.1f} games/s")
e.set_arena_openings(0)
e.close()
