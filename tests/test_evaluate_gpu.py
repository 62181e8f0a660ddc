"""Held-out loss on the GPU (az_net_evaluate, az_samples_holdout, az_net_train_set_validation / az_net_train_validation; include/az_engine.h,
csrc/az_score.h, DESIGN.md sections 4.1l and 8.3): the score kernel against the numpy twin (tests/score_twin.py) fed the device's own
az_net_predict_states output, at one row, at a chunk edge on either side and over several chunks with a ragged tail; the refusals; purity;
the hold-out mask; the per-epoch validation inside az_net_train and az_net_train_samples against runs of fewer epochs.  Every comparison
is bit for bit.  max_batch = 256 and net_channels = 128 throughout."""
import os
import sys

import numpy as np
import pytest
import torch                   # before the engine library is loaded: torch brings its own HIP runtime, and a process wants one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg       # noqa: E402
import score_twin as tw        # noqa: E402

pytestmark = pytest.mark.gpu

C, CHUNK = 128, 256
BAD, NO_MODEL = fg.AZ_ERR_BAD_ARGUMENT, 6
SIZES = [1, CHUNK - 1, CHUNK, CHUNK + 1, 1000]
CONV, HASH = 3, 10


@pytest.fixture(scope="module")
def sengine(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=CHUNK, net_channels=C)
    e.net_set_kind(10, engine_mod.NET_HASH, fg.HASH_SALT)
    e.net_set_kind(11, engine_mod.NET_HASH, fg.HASH_SALT)
    e.net_init_random(CONV, seed=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def window(sengine):
    """1000 tuples of a small self-play (both orientations; the moves past the temperature threshold have one-hot targets), every second z
    blended with a random root value, and draw weights with zeros among them."""
    r = sengine.selfplay(n_games=96, num_sims=10, model_id=HASH, seed=5, concurrent=48, temp_threshold=6)
    assert r["count"] >= 1000
    n = 1000
    states, boards, pis, zs = r["states"][:n].copy(), r["boards"][:n].copy(), r["pis"][:n].copy(), r["zs"][:n].copy()
    g = np.random.default_rng(8)
    zs[1::2] = (np.float32(0.5) * zs[1::2] + np.float32(0.5) * g.uniform(-1, 1, len(zs[1::2])).astype(np.float32)).astype(np.float32)
    assert (pis.max(axis=1) == 1).any() and (pis.max(axis=1) < 1).any() and (np.abs(zs) < 1).any()
    w = g.integers(0, 4, n).astype(np.uint32)
    w[0] = 2
    return {"states": states, "boards": boards, "pis": pis, "zs": zs, "w": w}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_matches_twin(got, want, n):
    assert got["sums"] == tuple(want["sums"])
    assert got["n"] == n and got["weight_sum"] == want["sums"][4]
    assert (got["loss_pi"], got["loss_v"], got["kl"], got["top1"]) == tw.results(want["sums"])
    for k, t in (("ce", "ce"), ("se", "se"), ("kl_rows", "kl")):
        assert np.array_equal(bits(got[k]), bits(want[t])), k


def check_model(e, model_id, win, n):
    """az_net_evaluate of the window's first n tuples against the twin on the device's own predict output: unweighted, weighted, by
    boards, by device pointers, and the weighted call against the window with tuple i repeated w_i times."""
    states, boards, pis, zs, w = (win[k][:n] for k in ("states", "boards", "pis", "zs", "w"))
    p, v = e.predict_states(states, model_id)
    want, want_w = tw.score_py(p, v, pis, zs, states), tw.score_py(p, v, pis, zs, states, w)
    got = e.evaluate(model_id, pis, zs, states=states, per_tuple=True)
    assert_matches_twin(got, want, n)
    got_w = e.evaluate(model_id, pis, zs, states=states, weights=w, per_tuple=True)
    assert_matches_twin(got_w, want_w, n)
    # the boards route
    by_boards = e.evaluate(model_id, pis, zs, boards=boards, weights=w, per_tuple=True)
    assert_matches_twin(by_boards, want_w, n)
    # device pointers in and out
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
    out = tuple(torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3))
    dev = e.evaluate(model_id, d(pis, np.float32), d(zs, np.float32), states=d(states, np.int64), weights=d(w, np.int32), out=out)
    dev["ce"], dev["se"], dev["kl_rows"] = (t.cpu().numpy() for t in out)
    assert_matches_twin(dev, want_w, n)
    # weights are multiplicities
    rep = np.repeat(np.arange(n), w)
    if len(rep):
        expanded = e.evaluate(model_id, pis[rep], zs[rep], states=states[rep])
        assert expanded["sums"] == got_w["sums"] and expanded["n"] == len(rep) == got_w["weight_sum"]
        assert all(expanded[k] == got_w[k] for k in ("loss_pi", "loss_v", "kl", "top1"))
    return got


@pytest.mark.parametrize("n", SIZES)
def test_scorer_equals_the_twin(sengine, engine_mod, window, n):
    """A random-init conv net in bf16, the same id pinned to fp8, "eval_mirror" on, and the hash net."""
    e = sengine
    bf16 = check_model(e, CONV, window, n)
    e.net_set_class(CONV, engine_mod.NET_CLASS_FP8)
    try:
        fp8 = check_model(e, CONV, window, n)
    finally:
        e.net_set_class(CONV, engine_mod.NET_CLASS_ENGINE)
    e.set_eval_mirror(True)
    try:
        mir = check_model(e, CONV, window, n)
    finally:
        e.set_eval_mirror(False)
    check_model(e, HASH, window, n)
    if n == 1000:              # the classes are different functions: the score tells them apart
        assert fp8["sums"] != bf16["sums"] and mir["sums"] != bf16["sums"]
    print("n %d: bf16 loss_pi %.6f loss_v %.6f kl %.6f top1 %.4f" % (n, bf16["loss_pi"], bf16["loss_v"], bf16["kl"], bf16["top1"]))


def test_refusals(sengine, engine_mod, window):
    e = sengine
    states, pis, zs = (window[k][:300].copy() for k in ("states", "pis", "zs"))

    def refused(status=BAD, model_id=HASH, **kw):
        args = dict(pis=pis, zs=zs, states=states)
        args.update(kw)
        ce = np.full(len(args["zs"]), 7.0, np.float32)
        with pytest.raises(engine_mod.AzError) as ei:
            e.evaluate(model_id, args["pis"], args["zs"], states=args["states"], weights=args.get("weights"), out=(ce, None, None))
        assert ei.value.status == status
        assert (ce == 7.0).all()                   # nothing written

    refused(pis=pis[:0], zs=zs[:0], states=states[:0])                                         # n = 0
    refused(weights=np.zeros(300, np.uint32))                                                  # W = 0
    heavy = np.ones(300, np.uint32)
    heavy[299] = (1 << 24) - 298
    refused(weights=heavy)                                                                     # W = 2^24 + 1
    heavy[299] -= 1
    assert e.evaluate(HASH, pis, zs, states=states, weights=heavy)["weight_sum"] == 1 << 24    # W = 2^24 is legal
    for bad in (-0.25, 1.5, np.nan):
        x = pis.copy()
        x[257, 3] = bad
        refused(pis=x)
    for bad in (-1.5, 1.25, np.nan):
        x = zs.copy()
        x[299] = bad
        refused(zs=x)
    x = states.copy()
    x[5] = (3, 1)                                                                              # overlapping stones
    refused(states=x)
    x = states.copy()
    x[280, 0] |= np.uint64(1 << 6)                                                             # a bit outside the board
    refused(states=x)
    planes = window["boards"][:10].copy()
    planes[4, 0, 5, 0] = planes[4, 1, 5, 0] = 1.0                                              # a cell set in both planes
    with pytest.raises(engine_mod.AzError) as ei:
        e.evaluate(HASH, pis[:10], zs[:10], boards=planes)
    assert ei.value.status == BAD
    refused(status=NO_MODEL, model_id=77)                                                      # an unknown id
    with pytest.raises(engine_mod.AzError):
        e.samples_holdout(0.25, 1, pis, zs, states=x)
    for key in ("train_keep_best", "train_patience"):                                          # refused without a registered set
        e.set_option(key, 1)
        try:
            with pytest.raises(engine_mod.AzError) as ei:
                e.train(CONV, 40, window["boards"][:64], pis[:64], zs[:64])
            assert ei.value.status == BAD
            with pytest.raises(engine_mod.AzError) as ei:
                e.train_samples(CONV, 40, pis[:64], zs[:64], states=states[:64])
            assert ei.value.status == BAD
        finally:
            e.set_option(key, 0)
    for key, v in (("train_keep_best", 2), ("train_patience", -1), ("train_patience", 1001)):
        with pytest.raises(engine_mod.AzError):
            e.set_option(key, v)


def test_evaluate_has_no_side_effects(sengine, window):
    """An arena, a tree batch and a shared slot give the same outputs before and after; no az_stats counter but device_ms moves."""
    e = sengine
    before = fg.other_entry_points(e)
    e.set_option("eval_cache_persist", 1)
    try:
        fg.arena_outputs(e)
        s0 = e.stats()
        for model_id in (HASH, CONV):
            e.evaluate(model_id, window["pis"], window["zs"], states=window["states"], weights=window["w"], per_tuple=True)
        e.samples_holdout(0.25, 3, window["pis"], window["zs"], states=window["states"])
        s1 = e.stats()
    finally:
        e.set_option("eval_cache_persist", 0)
    assert {k: v for k, v in s0.items() if k != "device_ms"} == {k: v for k, v in s1.items() if k != "device_ms"}
    fg.assert_same_outputs(fg.other_entry_points(e), before)


@pytest.mark.parametrize("n", [1, CHUNK + 1, 1000])
def test_holdout_equals_the_twin(sengine, window, n):
    e = sengine
    states, boards, pis, zs = (window[k][:n] for k in ("states", "boards", "pis", "zs"))
    for share, seed in ((0.25, 4), (0.5, 2 ** 63 + 11), (0.0, 4), (1.0, 4)):
        want = tw.holdout_py(states, share, seed)
        assert np.array_equal(e.samples_holdout(share, seed, pis, zs, states=states), want)
        assert np.array_equal(e.samples_holdout(share, seed, pis, zs, boards=boards), want)
    out = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    e.samples_holdout(0.25, 4, torch.from_numpy(pis).cuda(), torch.from_numpy(zs).cuda(), states=torch.from_numpy(states.view(np.int64)).cuda(), out=out)
    assert np.array_equal(out.cpu().numpy().astype(bool), tw.holdout_py(states, 0.25, 4))
    if n == 1000:              # the window holds both orientations of every position: each pair is on one side
        held = tw.holdout_py(states, 0.25, 4)
        assert np.array_equal(e.samples_holdout(0.25, 4, pis, zs, states=tw.mirror_states(states)), held) and 0 < held.sum() < n


# ---- per-epoch validation ------------------------------------------------------------------------------------------------------------------
class options:
    """Training options held for a block and put back to the engine's defaults behind it."""
    DEFAULTS = {"train_epochs": 10, "train_batch": 64, "train_seed": 0, "train_keep_best": 0, "train_patience": 0, "train_lr_e9": 1000000}

    def __init__(self, e, **kw):
        self.e, self.kw = e, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.e.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.e.set_option(k, self.DEFAULTS[k])


EPOCHS = 3


def run_training(e, win, weighted, **opts):
    """One az_net_train (or az_net_train_samples with weights) from CONV into slot 30 on tuples 0 .. 256 -> (params, loss history)."""
    t = slice(0, 256)
    with options(e, train_batch=64, train_seed=99, train_lr_e9=5000000, **opts):
        if weighted:
            hist = e.train_samples(CONV, 30, win["pis"][t], win["zs"][t], states=win["states"][t], weights=win["w"][t] + 1)
        else:
            hist = e.train(CONV, 30, win["boards"][t], win["pis"][t], win["zs"][t])
    return e.net_get_params(30), hist


@pytest.fixture(scope="module", params=[False, True], ids=["az_net_train", "az_net_train_samples"])
def shorter_runs(request, sengine, window):
    """Without a validation set: the models of 1, 2 and 3 epochs and az_net_evaluate of each on the 64-tuple validation set (tuples 300 ..
    364, weighted in the az_net_train_samples case).  The draw and mask streams are keyed by the global step: a shorter run is a prefix."""
    e, weighted = sengine, request.param
    v = slice(300, 364)
    val = dict(pis=window["pis"][v], zs=window["zs"][v], states=window["states"][v], weights=window["w"][v] + 1 if weighted else None)
    e.train_set_validation()
    runs = []
    for k in range(1, EPOCHS + 1):
        params, hist = run_training(e, window, weighted, train_epochs=k)
        assert len(hist) == k and e.train_validation() == ([], -1)
        s = e.evaluate(30, val["pis"], val["zs"], states=val["states"], weights=val["weights"])
        runs.append({"params": params, "hist": hist, "row": (s["loss_pi"], s["loss_v"], s["kl"], s["top1"])})
    assert not np.array_equal(runs[0]["params"], runs[1]["params"]) and len({r["row"] for r in runs}) == EPOCHS
    return weighted, val, runs


def test_validation_rows_are_the_shorter_runs(sengine, window, shorter_runs):
    e = sengine
    weighted, val, runs = shorter_runs
    e.train_set_validation(val["pis"], val["zs"], states=val["states"], weights=val["weights"])
    try:
        # both options off: every row is the evaluate of the shorter run, the stored model is the run's without a set
        params, hist = run_training(e, window, weighted, train_epochs=EPOCHS)
        rows, best = e.train_validation()
        print("validation rows", rows, "best", best)
        assert rows == [r["row"] for r in runs]
        assert hist == runs[-1]["hist"] and np.array_equal(params, runs[-1]["params"])
        assert best == tw.best_stop_py(rows, 0)[0]
        # the boards route registers the same set
        e.train_set_validation(val["pis"], val["zs"], boards=tw_boards(val["states"]), weights=val["weights"])
        run_training(e, window, weighted, train_epochs=2)
        assert e.train_validation()[0] == rows[:2]
        # keep the best epoch
        params, hist = run_training(e, window, weighted, train_epochs=EPOCHS, train_keep_best=1)
        assert e.train_validation() == (rows, best) and len(hist) == EPOCHS
        assert np.array_equal(params, runs[best]["params"])
        # patience 1: stop where the rule says; both histories have that length
        stop_at = next((k for k in range(1, EPOCHS + 1) if tw.best_stop_py(rows[:k], 1)[1]), EPOCHS)
        params, hist = run_training(e, window, weighted, train_epochs=EPOCHS, train_patience=1)
        got_rows, got_best = e.train_validation()
        assert got_rows == rows[:stop_at] and hist == runs[stop_at - 1]["hist"] and len(hist) == stop_at
        assert got_best == tw.best_stop_py(rows[:stop_at], 1)[0]
        assert np.array_equal(params, runs[stop_at - 1]["params"])
        params, _ = run_training(e, window, weighted, train_epochs=EPOCHS, train_patience=1, train_keep_best=1)
        assert np.array_equal(params, runs[got_best]["params"])
        # a set cannot change under an open session
        e.train_begin(CONV)
        try:
            with pytest.raises(Exception):
                e.train_set_validation()
        finally:
            e.train_end(31)
    finally:
        e.train_set_validation()
    run_training(e, window, weighted, train_epochs=1)
    assert e.train_validation() == ([], -1)


def tw_boards(states):
    from alphazero_rs_amd.coach import states_to_boards
    return states_to_boards(states)


# ---- the two Coaches -----------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_coach_agree_with_validation(engine_mod, tmp_path):
    """One iteration with validation_share = 0.25, keep_best and patience 1 on both hosts (the configuration of fg.run_coach_pair, 3
    epochs): the same report, the validation keys included, and byte-identical files; 0.examples is the plain run's (history is not
    split), 1.aznet is not."""
    import json
    import subprocess
    from alphazero_rs_amd.coach import Coach
    seed, epochs = 11, 3
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp", "plain")}

    def run_py(d, share, keep_best, patience):
        e = engine_mod.Engine(device=0, max_batch=CHUNK, net_channels=C)
        try:
            e.net_init_random(0, 3)
            e.set_option("train_epochs", epochs)
            coach = Coach.setup(e, d, 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 1, 32, 25, 1, 1000, 1, log=lambda m: None)
            coach.validation_share, coach.keep_best, coach.patience = share, keep_best, patience
            return coach.learn(seed=seed)
        finally:
            e.close()
    rep = run_py(dirs["py"], 0.25, True, 1)
    plain = run_py(dirs["plain"], 0.0, False, 0)
    exe = os.path.join(tmp_path, "test_coach_validation")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_validation.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, dirs["cpp"], str(C), str(seed), str(epochs), "0.25", "1", "1"], check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    crep = json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    assert len(rep) == len(crep) == 1
    r, c = rep[0], crep[0]
    print("python report", {k: r[k] for k in ("samples", "samples_raw", "val_n", "val_loss_pi", "val_loss_v", "val_top1", "best_epoch")})
    for k in fg.REPORT_KEYS + ("samples_raw", "val_n", "val_loss_pi", "val_loss_v", "val_top1", "best_epoch"):
        assert r[k] == c[k], k
    assert len(r["losses"]) == c["epochs"] == len(r["val_loss_pi"]) <= epochs
    assert 0 < r["val_n"] < r["samples_raw"] == r["samples"] + r["val_n"] == plain[0]["samples"]
    assert (r["best_epoch"], len(r["val_loss_pi"]) < epochs) == tw.best_stop_py(list(zip(r["val_loss_pi"], r["val_loss_v"])), 1) or len(r["val_loss_pi"]) == epochs
    fg.compare_directories(dirs["py"], dirs["cpp"])
    read = lambda d, f: open(os.path.join(dirs[d], f), "rb").read()
    assert read("py", "0.examples") == read("plain", "0.examples")
    assert read("py", "1.aznet") != read("plain", "1.aznet")
    assert "val_n" not in plain[0]
