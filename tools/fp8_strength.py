"""Does the fp8 class play worse?  The same TRAINED parameters in two model ids of one engine, one pinned BF16, one FP8
(az_net_set_class), compared two ways:
  move agreement  100-simulation temp-0 searches from at least 2000 distinct positions of the run's own self-play samples, rooted with
                  az_tree_reset: the share of equal moves, and mean / max |d pi| of the visit distributions (counts / sum)
  arena           ONE 98-game az_arena over a 49-entry opening book (az_arena_set_opening_book: the 49 two-ply openings), fp8 (new) against
                  bf16 (old): pair p plays opening p in both seatings.  At temp 0 the games of an arena from one position differ only by
                  tie-breaks, so a call from the empty board is two games, not a sample: the openings are what makes 98 different games.
                  A bf16-against-bf16 control of the same shape gives the tally a pair of equal players produces.
The input is the checkpoint directory of a short run of examples/connect_four.py (a random-init net has near-uniform priors and says
nothing):  python examples/connect_four.py --checkpoint D --iters 3 --eps 1024 --sims 50 --slots 1024 --arena 32 --epochs 4
           python tools/fp8_strength.py D [--positions 2000] [--sims 100]"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_rs_amd import engine as azeng
from alphazero_rs_amd.coach import load_examples, read_state

ap = argparse.ArgumentParser()
ap.add_argument("checkpoint")
ap.add_argument("--positions", type=int, default=2000)
ap.add_argument("--sims", type=int, default=100)
a = ap.parse_args()
it, live = read_state(a.checkpoint)
weights = os.path.join(a.checkpoint, f"{live}.aznet")
channels = int(np.fromfile(weights, np.int64, 1, offset=8)[0])
# distinct positions of the run's samples: feature planes [2][6][7] (row 0 = top) -> canonical bitboards; every sample is a position a
# move was chosen from, so it is legal and not finished
boards = np.concatenate([h[0] for h in load_examples(os.path.join(a.checkpoint, f"{it}.examples"))])
bits = np.array([[1 << (c * 7 + (5 - r)) for c in range(7)] for r in range(6)], dtype=np.uint64)
states = np.stack([(boards[:, p] != 0).astype(np.uint64).reshape(-1, 42) @ bits.reshape(42) for p in (0, 1)], axis=1)
states = np.unique(states, axis=0)
states = states[np.random.default_rng(0).permutation(len(states))[: a.positions]]
assert len(states) >= min(a.positions, 2000), f"only {len(states)} distinct positions in the run: play more episodes"
G = len(states)
e = azeng.Engine(device=0, max_batch=max(G, 256), net_channels=channels)
for mid, cls in ((0, azeng.NET_CLASS_BF16), (1, azeng.NET_CLASS_FP8), (2, azeng.NET_CLASS_BF16)):
    e.net_load(mid, weights)
    e.net_set_class(mid, cls)
res = {}
for mid in (0, 1):
    t = e.tree_create(G, 1000000, a.sims, 1000, mid, 1)
    t.reset(states)
    pi, counts, q = t.get_action_prob(states, 0.0, seed=1)
    t.close()
    res[mid] = (pi.argmax(axis=1), counts.astype(np.float64) / counts.sum(axis=1, keepdims=True))
dpi = np.abs(res[0][1] - res[1][1]).max(axis=1)
agree = float((res[0][0] == res[1][0]).mean())
print(f"net {weights} (C = {channels}), {G} distinct positions, {a.sims} simulations, temp 0")
print(f"move agreement fp8 / bf16: {agree:.4f} ({int((res[0][0] != res[1][0]).sum())} of {G} differ); |d pi| of the visit distributions: mean {dpi.mean():.4f} max {dpi.max():.4f}")


def openings():
    for c1 in range(7):
        for c2 in range(7):
            yield c1, c2, (1 << (c1 * 7), 1 << (c2 * 7 + (1 if c1 == c2 else 0)))        # (first seat's stones, second seat's stones)


tally = {}
e.arena_set_opening_book([sb for _, _, sb in openings()])
for name, new_id in (("fp8 vs bf16", 1), ("bf16 vs bf16 (control)", 2)):
    w, _ = e.arena(98, a.sims, new_model_id=new_id, old_model_id=0, seed=1000)
    wld = w.astype(np.int64)
    tally[name] = wld.tolist()
    print(f"arena over the 49 two-ply openings x both seatings, {name}: W/L/D of the first-named = {wld[0]} / {wld[1]} / {wld[2]}")
e.close()
print(json.dumps({"positions": G, "sims": a.sims, "move_agreement": agree, "dpi_mean": float(dpi.mean()), "dpi_max": float(dpi.max()), "arena_wld": tally}))
