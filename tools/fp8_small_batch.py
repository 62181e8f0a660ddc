"""Device time of an fp8 model's conv3, conv4 and whole forward at arena-size batches (1, 20, 32, 64, 128 boards by default), from the
engine's HIP-event brackets, with "narrow_rows" at 32 (small batches on k_gemm_skinny_f8) and at 0 (the LDS-DMA ring at every size).
python tools/fp8_small_batch.py [--root TREE] [--reps 200] [boards ...]
--root: import the package of ANOTHER checkout (an A/B partner built beside this one); the script only uses "net_fp8" and
"narrow_rows", so it also runs on a tree whose fp8 path has no small-batch kernel (both columns then time the ring).
Prints one line per (boards, narrow_rows) and a last JSON line {"conv34_us": {"<boards>/<narrow_rows>": us}}."""
import argparse, json, os, sys
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--channels", type=int, default=512)
ap.add_argument("boards", nargs="*", type=int)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
from alphazero_rs_amd import engine as azeng
from tools._states import random_states
boards = a.boards or [1, 20, 32, 64, 128]
e = azeng.Engine(device=0, max_batch=256, net_channels=a.channels, profile=True)
e.net_init_random(0, seed=1)
e.set_option("net_fp8", 1)
st = random_states(max(boards), seed=3)
out = {}
for n in boards:
    for nr in (32, 0):
        e.set_option("narrow_rows", nr)
        for _ in range(20):
            e.predict_states(st[:n], 0)
        e.reset_stats()
        for _ in range(a.reps):
            e.predict_states(st[:n], 0)
        s = e.stats()
        L = max(1, s["net_launches"])
        c3, c4, tot = (s[k] / L * 1e3 for k in ("net_conv3_ms", "net_conv4_ms", "net_total_ms"))
        out[f"{n}/{nr}"] = round(c3 + c4, 2)
        print("boards %4d  narrow_rows %2d  conv3 %6.1f  conv4 %6.1f  conv3+conv4 %6.1f  whole forward %6.1f us  (%d forwards)" % (n, nr, c3, c4, c3 + c4, tot, L), flush=True)
e.close()
print(json.dumps({"root": os.path.abspath(a.root), "conv34_us": out}))
