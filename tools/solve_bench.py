"""The exact endgame solver (az_solve) measured on self-play positions: conv net with random weights, C = 512, 8192
episodes, 100 sims/move.  GPU only; nothing here is a pass/fail threshold.
For the positions with at least 22, 18 and 14 stones (a seeded sample of `sample`, `sample` / 4 and `sample` / 16 distinct ones: the
searches grow by an order of magnitude every four stones), for tt_log2 0 / 12 / 16 and max_nodes 2^20 / 2^24: wall time of the call
(host arrays in and out, best of 2 behind a warm-up call that sizes the workspaces), items/s, nodes/s, mean and maximum nodes per
searched item and the UNKNOWN share of the legal items.  Then the grid cap (max_lanes) at tt_log2 12, and the same items on the g++
twin (tests/cpp/solve_twin.cpp, one CPU core) for the CPU's nodes/s.  Configurations are run cheapest first and the ones that would start
behind `budget_s` seconds are skipped and listed.
part = grid: only the grid cap on the sample, and ALL distinct positions with at least 22 stones in one call (the machine filled).
python tools/solve_bench.py [episodes=8192] [sims=100] [channels=512] [sample=4096] [budget_s=420] [part=all|grid]"""
import os, sys, time
import numpy as np
import torch                   # before the engine library: one HIP runtime per process
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from alphazero_rs_amd import engine as azeng
import solve_twin
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
episodes, sims, channels, sample, budget_s, part = arg(1, 8192), arg(2, 100), arg(3, 512), arg(4, 4096), arg(5, 420), arg(6, "all", str)
T0 = time.perf_counter()


def popcount(x):
    return np.array([bin(int(v)).count("1") for v in x])


def timed(e, pos, **kw):
    e.solve(pos[:64], **kw)
    best = None
    for _ in range(2):
        t = time.perf_counter()
        mv, v, nodes = e.solve(pos, **kw)
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best, mv, nodes


def row(tag, dt, mv, nodes):
    legal = mv != azeng.SOLVE_ILLEGAL
    searched = nodes > 0
    print(f"{tag}: {dt * 1e3:9.1f} ms  items/s {legal.sum() / dt:11.0f}  nodes/s {nodes.sum() / dt:13.0f}  nodes/searched item mean "
          f"{nodes[searched].mean() if searched.any() else 0:10.1f} max {nodes.max():9d}  UNKNOWN {(mv == azeng.SOLVE_UNKNOWN).sum() / max(1, legal.sum()):.4f}", flush=True)


def main():
    e = azeng.Engine(device=0, max_batch=8192, net_channels=channels)
    e.net_init_random(0, 0)
    t = time.perf_counter()
    r = e.selfplay(n_games=episodes, concurrent=episodes, num_sims=sims, model_id=0, seed=1, symmetries=False, want_boards=False)
    states = np.unique(r["states"], axis=0)
    stones = popcount(states[:, 0] | states[:, 1])
    print(f"self-play: {episodes} episodes, {sims} sims: {r['count']} positions, {len(states)} distinct, in {time.perf_counter() - t:.1f} s", flush=True)
    rng = np.random.default_rng(0)
    sets = {}
    for lo, k in ((22, sample), (18, sample // 4), (14, sample // 16)):
        idx = np.flatnonzero(stones >= lo)
        pick = rng.choice(idx, size=min(k, len(idx)), replace=False)
        sets[lo] = np.ascontiguousarray(states[np.sort(pick)])
        print(f"  >= {lo} stones: {len(idx)} distinct positions, {len(sets[lo])} sampled, mean stones {stones[pick].mean():.1f}", flush=True)
    skipped = []
    configs = [(lo, tt, mn) for mn in (1 << 20, 1 << 24) for lo in (22, 18, 14) for tt in (16, 12, 0)] if part == "all" else []
    if part == "grid":
        everything = np.ascontiguousarray(states[stones >= 22])
        for tt in (12, 16):
            dt, mv, nodes = timed(e, everything, max_nodes=1 << 20, tt_log2=tt)
            row(f"all {len(everything)} positions >= 22 stones  tt_log2 {tt:2d}  max_nodes 2^20", dt, mv, nodes)
    for lo, tt, mn in configs:
        if time.perf_counter() - T0 > budget_s:
            skipped.append((lo, tt, mn))
            continue
        dt, mv, nodes = timed(e, sets[lo], max_nodes=mn, tt_log2=tt)
        row(f">= {lo} stones  tt_log2 {tt:2d}  max_nodes 2^{mn.bit_length() - 1}", dt, mv, nodes)
    for lanes in (64, 4096, 16384, 65536, 0):
        if time.perf_counter() - T0 > budget_s:
            skipped.append(("lanes", lanes))
            continue
        dt, mv, nodes = timed(e, sets[22], max_nodes=1 << 20, tt_log2=12, max_lanes=lanes)
        row(f">= 22 stones  tt_log2 12  max_nodes 2^20  max_lanes {lanes:6d}", dt, mv, nodes)
    for lo, k in ((22, 1024), (18, 64)) if part == "all" else ():
        pos = sets[lo][:k]
        t = time.perf_counter()
        mv, v, nodes = solve_twin.twin(pos, 0, 1 << 20, 0, 12)
        dt = time.perf_counter() - t
        row(f"g++ twin, one core, >= {lo} stones ({len(pos)} positions)  tt_log2 12  max_nodes 2^20", dt, mv, nodes)
    if skipped:
        print("skipped (time budget):", skipped)
    e.close()


main()
