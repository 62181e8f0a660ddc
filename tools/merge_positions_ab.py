"""Position averaging (az_samples_merge) measured at the Coach configuration README quotes: conv net, C = 512, 8192
episodes, 100 sims/move, symmetries expanded at the destination as both Coaches do.  GPU only; nothing here is a pass/fail threshold.
  A  m / n of one iteration's tuples, with and without AZ_MERGE_CANONICAL, without and with Dirichlet root noise (eps 0.25, alpha 1)
  B  wall time of the call against n (device pointers in and out, so no host copy is in it; best and median of `reps` calls behind a
     warm-up that sizes the workspace) on three inputs: all distinct, all identical (the contention worst case), the self-play set.
     "All distinct" are random disjoint bit patterns, not reachable positions: Game::pack is an identity for stacked stones only, so a
     few of them share a key (m is printed)
  C  the merge as both Coaches call it (feature planes in pageable host memory in, planes back out: wall time of Engine.merge_samples,
     best of 3), then az_net_train seconds on the raw set and on the merged set (`epochs` epochs each; steps = epochs * n / batch)
  D  the weighted arm (az_net_train_samples): az_net_train on the raw set, on the merged set, and
     az_net_train_samples on the merged STATES with the counts as weights (mirrored at random under AZ_MERGE_CANONICAL) -- seconds, ms per
     step and the last epoch's training losses.  The losses are each route's own: merged targets are means, so their cross-entropy floor
     is higher than the raw one-game targets' even where the gradients agree in expectation
python tools/merge_positions_ab.py A|B|C|D [episodes=8192] [sims=100] [channels=512] [epochs=2] [reps=5]"""
import os, sys, time
import numpy as np
import torch                   # before the engine library: one HIP runtime per process
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_rs_amd import engine as azeng
from alphazero_rs_amd.coach import states_to_boards
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
part, episodes, sims, channels, epochs, reps = arg(1, "A", str), arg(2, 8192), arg(3, 100), arg(4, 512), arg(5, 2), arg(6, 5)
FULL = sum(0x3F << (7 * c) for c in range(7))


def mirror_bits(b):
    r = np.zeros_like(b)
    for c in range(7):
        r |= ((b >> np.uint64(7 * c)) & np.uint64(0x7F)) << np.uint64(7 * (6 - c))
    return r


def iteration_tuples(e, noise):
    """One Coach iteration's window: az_selfplay without symmetries, identity + mirror image per tuple at the destination."""
    if noise:
        e.set_root_noise(0.25, 1.0)
    t = time.perf_counter()
    r = e.selfplay(n_games=episodes, concurrent=episodes, num_sims=sims, model_id=0, seed=1, symmetries=False, want_boards=False)
    dt = time.perf_counter() - t
    e.set_root_noise(0.0, 1.0)
    s, p, z = r["states"], r["pis"], r["zs"]
    s2 = np.empty((2 * len(z), 2), np.uint64); p2 = np.empty((2 * len(z), 7), np.float32)
    s2[0::2], s2[1::2] = s, np.stack([mirror_bits(s[:, 0]), mirror_bits(s[:, 1])], axis=1)
    p2[0::2], p2[1::2] = p, p[:, ::-1]
    print(f"self-play: {episodes} episodes, {sims} sims, root noise {int(noise)}: {len(z)} tuples ({2 * len(z)} with symmetries) in {dt:.2f} s", flush=True)
    return s2, p2, np.repeat(z, 2)


def timed_merge(e, s, p, z, canonical):
    """The bare call on device tensors -> (m, seconds of each of `reps` calls)."""
    dev = torch.device("cuda", 0)
    n = len(z)
    ts, tp, tz = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s.view(np.int64), p, z))
    os_, op, oz, oc = (torch.empty((n,) + sh, dtype=dt, device=dev) for sh, dt in (((2,), torch.int64), ((7,), torch.float32), ((), torch.float32), ((), torch.int32)))
    src = azeng.az_samples(n, n, azeng._as_ptr(ts), None, azeng._as_ptr(tp), azeng._as_ptr(tz), None, None)
    dst = azeng.az_samples(n, 0, azeng._as_ptr(os_), None, azeng._as_ptr(op), azeng._as_ptr(oz), None, None)
    secs = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        e._check(e._lib.az_samples_merge(e._h, azeng.C.byref(src), 1 if canonical else 0, azeng.C.byref(dst), azeng._as_ptr(oc)))
        secs.append(time.perf_counter() - t)
    return int(dst.count), secs[1:]


e = azeng.Engine(device=0, max_batch=max(episodes, 256), net_channels=channels)
e.net_init_random(0, 1)
e.selfplay(n_games=256, concurrent=256, num_sims=25, model_id=0, want_boards=False)        # warm-up
if part == "A":
    for noise in (False, True):
        s, p, z = iteration_tuples(e, noise)
        for canonical in (False, True):
            r = e.merge_samples(p, z, states=s, canonical=canonical)
            c = r["counts"]
            print(f"A  root noise {int(noise)} canonical {int(canonical)}: n {len(z)}  m {r['count']}  m/n {r['count'] / len(z):.4f}  "
                  f"largest group {int(c.max())}  groups of one {int((c == 1).sum())}  tuples in groups of one {int((c == 1).sum()) / len(z):.4f}", flush=True)
elif part == "B":
    rng = np.random.default_rng(0)
    sp = iteration_tuples(e, False)
    for log2n in (16, 18, 20, 22, 24):
        n = 1 << log2n
        p = rng.random((n, 7), dtype=np.float32); p /= p.sum(axis=1, keepdims=True)
        z = rng.choice(np.array([1, -1, 1e-4], np.float32), n)
        mine = rng.integers(0, 1 << 48, n, dtype=np.uint64) & np.uint64(FULL)
        theirs = rng.integers(0, 1 << 48, n, dtype=np.uint64) & np.uint64(FULL) & ~mine
        for name, s in (("all distinct", np.stack([mine, theirs], axis=1)), ("all identical", np.zeros((n, 2), np.uint64))):
            m, secs = timed_merge(e, s, p, z, False)
            print(f"B  {name:13s} n 2^{log2n}  m {m}  best {min(secs) * 1e3:9.3f} ms  median {sorted(secs)[len(secs) // 2] * 1e3:9.3f} ms  "
                  f"{n / min(secs) / 1e6:8.1f} M tuples/s", flush=True)
    for canonical in (False, True):
        m, secs = timed_merge(e, *sp, canonical)
        print(f"B  self-play set canonical {int(canonical)}  n {len(sp[2])}  m {m}  best {min(secs) * 1e3:9.3f} ms  median {sorted(secs)[len(secs) // 2] * 1e3:9.3f} ms  "
              f"{len(sp[2]) / min(secs) / 1e6:8.1f} M tuples/s", flush=True)
elif part == "C":
    s, p, z = iteration_tuples(e, False)
    e.set_option("train_epochs", epochs)
    sets = [("raw", states_to_boards(s), p, z)]
    for canonical in (False, True):
        secs = []
        for _ in range(4):
            t = time.perf_counter()
            r = e.merge_samples(p, z, boards=sets[0][1], canonical=canonical, want_boards=True)
            secs.append(time.perf_counter() - t)
        print(f"C  Coach route (host planes in, planes out) canonical {int(canonical)}: n {len(z)}  m {r['count']}  merge_samples best {min(secs[1:]) * 1e3:.1f} ms  "
              f"first call {secs[0] * 1e3:.1f} ms", flush=True)
        sets.append((f"merged canonical {int(canonical)}", r["boards"], r["pis"], r["zs"]))
    for name, b, pp, zz in sets:
        t = time.perf_counter()
        losses = e.train(0, 1, b, pp, zz)
        dt = time.perf_counter() - t
        steps = epochs * (len(zz) // 64)
        print(f"C  {name:18s} n {len(zz)}  {epochs} epochs  {steps} steps  az_net_train {dt:8.2f} s  {dt / max(steps, 1) * 1e3:.3f} ms/step  last loss {losses[-1]}", flush=True)
elif part == "D":
    s, p, z = iteration_tuples(e, False)
    e.set_option("train_epochs", epochs)

    def report(name, n, fn):
        t = time.perf_counter()
        losses = fn()
        dt = time.perf_counter() - t
        steps = epochs * max(1, n // 64)
        print(f"D  {name:28s} n {n}  {epochs} epochs  {steps} steps  {dt:8.2f} s  {dt / steps * 1e3:.3f} ms/step  last loss {losses[-1]}", flush=True)
    report("raw az_net_train", len(z), lambda: e.train(0, 1, states_to_boards(s), p, z))
    for canonical in (False, True):
        r = e.merge_samples(p, z, states=s, canonical=canonical)
        m = r["count"]
        print(f"D  canonical {int(canonical)}: n {len(z)}  m {m}  sum of counts {int(r['counts'].sum(dtype=np.uint64))}", flush=True)
        report(f"merged c{int(canonical)} az_net_train", m, lambda: e.train(0, 1, states_to_boards(r["states"]), r["pis"], r["zs"]))
        report(f"merged c{int(canonical)} weighted", m, lambda: e.train_samples(0, 1, r["pis"], r["zs"], states=r["states"], weights=r["counts"], mirror=canonical))
e.close()
