"""The decided-move stop (include/az_search_stop.h) on one GPU with randomly initialised conv nets: feature on against
off on the SAME engine, in alternating rounds.  A measurement, no pass/fail bar.
Workloads: arena = bench.py's arena shape (`games` games x `sims` simulations, two nets); tournament = az_tournament of 4 models x `games`
games per pair; selfplay = `games` slots x `sims` simulations, 2 x `games` episodes, the example's temp_threshold 15.  One warm-up call of
each shape and setting first (tree arenas, graph captures).  Per workload and setting: games/s of every round, leaf_rows_requested /
leaf_rows_executed and simulations of the last round, the four counters, and -- from one more call of each setting with the profile
brackets on ("profile" 1, every 16th step) -- the mean time of a tree launch (k_backup_select).  One JSON line per workload.
python tools/search_stop_ab.py [workload=all] [rounds=3] [arena_games=4096] [arena_sims=400] [tournament_games=512] [selfplay_slots=8192]
                               [selfplay_sims=100] [channels=512]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401  (before the engine library is loaded: a process wants one HIP runtime)
from alphazero_rs_amd import engine as azeng
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
workload, rounds, a_games, a_sims, t_games, s_slots, s_sims, channels = (arg(1, "all", str), arg(2, 3), arg(3, 4096), arg(4, 400), arg(5, 512), arg(6, 8192),
                                                                         arg(7, 100), arg(8, 512))
SEED = 1


def engine(max_batch, models):
    e = azeng.Engine(device=0, max_batch=max_batch, net_channels=channels)
    for i, m in enumerate(models):
        e.net_init_random(m, SEED + i)
    return e


def measure(name, e, call, games):
    """call(seed) plays one call of the workload; on / off alternate, the warm-up calls first."""
    out = {"workload": name, "games_per_call": games, "rounds": rounds, "on": {"games_per_sec": []}, "off": {"games_per_sec": []}}
    for on in (0, 1):
        e.set_search_stop(on)
        call(SEED + 7)
    for r in range(rounds):
        for on in ((0, 1) if r % 2 == 0 else (1, 0)):
            e.set_search_stop(on)
            e.reset_stats()
            e.search_stop_stats(reset=True)
            t = time.perf_counter()
            call(SEED)
            dt = time.perf_counter() - t
            s, side = e.stats(), out["on" if on else "off"]
            side["games_per_sec"].append(round(games / dt, 2))
            side.update(leaf_rows_requested=s["leaf_rows_requested"], leaf_rows_executed=s["leaf_rows_executed"], simulations=s["simulations"],
                        tree_launches=s["tree_launches"], counters=e.search_stop_stats())
    e.set_option("profile_every", 16)
    for on in (0, 1):                       # the profile pass: its wall time is not a result (the brackets idle the device and preclude graphs)
        e.set_search_stop(on)
        e.set_option("profile", 1)
        e.reset_stats()
        call(SEED)
        s = e.stats()
        e.set_option("profile", 0)
        out["on" if on else "off"]["tree_launch_mean_us"] = round(1e3 * s["tree_ms"] / max(1, s["tree_launches_timed"]), 2)
    e.set_search_stop(0)
    for side in ("on", "off"):
        g = out[side]["games_per_sec"]
        out[side]["best"], out[side]["spread"] = max(g), round(max(g) - min(g), 2)
    out["speedup_best"] = round(out["on"]["best"] / out["off"]["best"], 4)
    c = out["on"]["counters"]
    out["skipped_share_of_eligible_budget"] = round(c["skipped_sims"] / max(1, c["budgeted_sims"]), 4)
    print(json.dumps(out), flush=True)
    return out


if workload in ("all", "arena"):
    e = engine(a_games, (0, 2))
    measure("arena", e, lambda seed: e.arena(num_games=a_games, num_sims=a_sims, new_model_id=2, old_model_id=0, seed=seed), a_games)
    e.close()
if workload in ("all", "tournament"):
    e = engine(3 * t_games, (0, 1, 2, 3))
    measure("tournament", e, lambda seed: e.tournament([0, 1, 2, 3], t_games, a_sims, seed=seed), 6 * t_games)
    e.close()
if workload in ("all", "selfplay"):
    e = engine(s_slots, (0,))
    measure("selfplay", e, lambda seed: e.selfplay(n_games=2 * s_slots, concurrent=s_slots, num_sims=s_sims, model_id=0, seed=seed, temp_threshold=15,
                                                   want_boards=False), 2 * s_slots)
    e.close()
