"""Held-out loss on the device (az_net_evaluate, az_net_train_set_validation; csrc/az_score.h, DESIGN.md sections 4.1l and 8.3) on one GPU with
a randomly initialised conv net.  A measurement, no pass/fail bar.
mode "score": az_net_evaluate on a self-play window of `window` tuples by the states route with device arrays, in bf16 and in fp8, against
the route there was before it -- az_net_predict_states over the window plus host arithmetic in numpy (float64 cross-entropy, squared error
and top-1 among the legal moves).  Best of `rounds` calls each; the first call sizes the workspace and is not counted.
mode "train": az_net_train on `train_n` tuples for `epochs` epochs without and with a validation set of `share` of them, in alternating
rounds: the seconds per epoch the validation adds.
mode "kernels": `rounds` az_net_evaluate calls and nothing else behind the warm-up -- for a kernel-stats run of a profiler, which then
shows the score kernel's share of the device time.
python tools/evaluate_bench.py [mode=score] [window=372000] [channels=512] [max_batch=8192] [rounds=3] [train_n=200000] [epochs=2] [share=0.05]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from alphazero_rs_amd import engine as azeng
from alphazero_rs_amd.coach import states_to_boards
arg = lambda i, d, t=int: t(sys.argv[i]) if len(sys.argv) > i else d
mode, window, channels, max_batch, rounds, train_n, epochs, share = (arg(1, "score", str), arg(2, 372000), arg(3, 512), arg(4, 8192), arg(5, 3),
                                                                     arg(6, 200000), arg(7, 2), arg(8, 0.05, float))
SEED = 1

e = azeng.Engine(device=0, max_batch=max_batch, net_channels=channels)
e.net_init_random(0, SEED)
games = 2048
res = e.selfplay(n_games=games, concurrent=min(games, max_batch), num_sims=25, model_id=0, seed=SEED, want_boards=False)
need = max(window, train_n)
idx = np.arange(need) % res["count"]
states, pis, zs = res["states"][idx], res["pis"][idx], res["zs"][idx]
print(f"window: {res['count']} self-play tuples of {games} episodes, repeated to {need}", flush=True)


def host_score(p, v, pis, zs, states):
    """What a host could do with az_net_predict_states' output: float64 means (not the engine's fixed-point sums)."""
    p64, pi64 = np.maximum(p.astype(np.float64), 2.0 ** -126), pis.astype(np.float64)
    ce = -np.where(pis >= np.float32(2.0 ** -126), pi64 * np.log(p64), 0.0).sum(axis=1)
    se = (v.astype(np.float64) - zs.astype(np.float64)) ** 2
    occ = states[:, 0] | states[:, 1]
    legal = np.stack([(occ >> np.uint64(c * 7 + 5)) & np.uint64(1) == 0 for c in range(7)], axis=1)
    hit = np.argmax(pis, axis=1) == np.argmax(np.where(legal, p, -1.0), axis=1)
    return float(ce.mean()), float(se.mean()), float(hit.mean())


if mode in ("score", "kernels"):
    s, p, z = states[:window], pis[:window], zs[:window]
    d_s, d_p, d_z = torch.from_numpy(s.view(np.int64)).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(z).cuda()
    for name, klass in (("bf16", azeng.NET_CLASS_BF16), ("fp8", azeng.NET_CLASS_FP8)):
        e.net_set_class(0, klass)
        e.evaluate(0, d_p, d_z, states=d_s)                             # sizes the workspace
        best_wall, best_dev = 1e30, 1e30
        for r in range(rounds):
            e.reset_stats()
            t = time.perf_counter()
            got = e.evaluate(0, d_p, d_z, states=d_s)
            best_wall = min(best_wall, time.perf_counter() - t)
            best_dev = min(best_dev, e.stats()["device_ms"])
        print(f"az_net_evaluate {name}: {window} tuples, {1e3 * best_wall:9.2f} ms wall, {best_dev:9.2f} ms inside the engine, {window / best_wall:10.0f} rows/s; "
              f"loss_pi {got['loss_pi']:.6f} loss_v {got['loss_v']:.6f} kl {got['kl']:.6f} top1 {got['top1']:.4f}", flush=True)
        if mode == "kernels":
            continue
        best_pred, best_host = 1e30, 1e30
        for r in range(rounds):
            t = time.perf_counter()
            pp, vv = e.predict_states(s, 0)
            t1 = time.perf_counter()
            ref = host_score(pp, vv, p, z, s)
            best_pred, best_host = min(best_pred, t1 - t), min(best_host, time.perf_counter() - t1)
        print(f"az_net_predict_states + numpy {name}: predict {1e3 * best_pred:9.2f} ms, host arithmetic {1e3 * best_host:9.2f} ms, "
              f"{window / (best_pred + best_host):10.0f} rows/s; loss_pi {ref[0]:.6f} loss_v {ref[1]:.6f} top1 {ref[2]:.4f}; "
              f"az_net_evaluate is {(best_pred + best_host) / best_wall:.2f} x faster", flush=True)
    e.net_set_class(0, azeng.NET_CLASS_ENGINE)

if mode == "train":
    n_val = int(round(train_n * share))
    b, p, z = states_to_boards(states[:train_n]), pis[:train_n], zs[:train_n]
    vs, vp, vz = states[train_n - n_val:train_n], pis[train_n - n_val:train_n], zs[train_n - n_val:train_n]     # timing only: the set overlaps the window
    e.set_option("train_epochs", epochs)
    times = {False: [], True: []}
    for r in range(rounds):
        for on in (False, True):
            if on:
                e.train_set_validation(vp, vz, states=vs)
            else:
                e.train_set_validation()
            t = time.perf_counter()
            hist = e.train(0, 1, b, p, z)
            dt = time.perf_counter() - t
            times[on].append(dt)
            extra = f" validation rows {e.train_validation()[0]}" if on else ""
            print(f"az_net_train round {r} validation {'on ' if on else 'off'}: {dt:8.3f} s for {epochs} epochs of {train_n // 64} steps{extra}", flush=True)
    e.train_set_validation()
    off, on = min(times[False]), min(times[True])
    print(f"az_net_train {train_n} tuples, {epochs} epochs, validation set {n_val}: best of {rounds} off {off:.3f} s, on {on:.3f} s: "
          f"{(on - off) / epochs:+.3f} s per epoch ({100.0 * (on - off) / off:+.2f} %); spread off {max(times[False]) - off:.3f} s, on {max(times[True]) - on:.3f} s")
e.close()
