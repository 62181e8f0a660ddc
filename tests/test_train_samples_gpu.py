"""Multiplicity-weighted training draws on the GPU (az_net_train_samples / az_net_train_draw, include/az_engine.h; csrc/az_draw.h, DESIGN.md
section 8.2): the device prefix sum and draw kernel against the numpy twin (tests/train_draw_twin.py) at the scan's block boundaries, the
trainer entry bit for bit against az_net_train and against a hand replay through the step entry, the refusals, purity, and both Coaches.
Everything runs at net_channels = 128, the width tests/test_train_gpu.py uses."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch                   # before the engine library is loaded: torch brings its own HIP runtime, and a process wants one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg       # noqa: E402
import train_draw_twin as tw   # noqa: E402

pytestmark = pytest.mark.gpu

C = 128
BAD = fg.AZ_ERR_BAD_ARGUMENT


def scan_constants():
    """B, the weights one workgroup of the scan's first and third pass takes, and G, the block sums one round of the second pass takes."""
    hdr = open(os.path.join(ROOT, "alphazero-rs_amd", "csrc", "az_draw.h")).read()
    val = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, hdr).group(1))
    return val("DRAW_SCAN_THREADS") * val("DRAW_SCAN_ITEMS"), val("DRAW_SCAN_GROUP")


B, G = scan_constants()


@pytest.fixture(scope="module")
def tengine(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=1024, net_channels=C)
    yield e
    e.close()


def make_set(n, seed):
    """n positions with stones stacked from the bottom (states and the matching planes), a pi on the simplex, z in {-1, 1, 1e-4}."""
    rng = np.random.default_rng(seed)
    states = np.zeros((n, 2), np.uint64)
    for i in range(n):
        for col in range(7):
            for r in range(rng.integers(0, 7)):
                states[i, rng.integers(0, 2)] |= np.uint64(1 << (col * 7 + r))
    logits = rng.normal(size=(n, 7))
    pis = (np.exp(logits) / np.exp(logits).sum(axis=1, keepdims=True)).astype(np.float32)
    vs = rng.choice([-1.0, 1.0, 1e-4], size=n).astype(np.float32)
    return states, tw.states_to_boards(states), pis, vs


class options:
    """Training options held for a block and put back to the engine's defaults behind it."""
    DEFAULTS = {"train_epochs": 10, "train_batch": 64, "train_seed": 0, "train_graph": 1}

    def __init__(self, e, **kw):
        self.e, self.kw = e, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.e.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.e.set_option(k, self.DEFAULTS[k])


# ---- 5. the scan and the draw kernel against the twin ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, B - 1, B, B + 1, B * G + 1])
def test_draw_equals_the_twin(tengine, n):
    """Index for index and mirror bit for mirror bit: all-ones weights, random u32 weights with zeros, one weight of 2^32 - 1 among
    ones, and NULL; t0 > 0; host and device pointers.  B * G + 1 weights are the fewest at which the scan of the block sums takes a
    second round."""
    e, batch, steps, seed = tengine, 32, 64, 4242 + n
    rng = np.random.default_rng(n)
    rand = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    rand[rng.random(n) < 0.25] = 0
    if not rand.any():
        rand[rng.integers(0, n)] = 7
    heavy = np.ones(n, np.uint32)
    heavy[rng.integers(0, n)] = 0xFFFFFFFF
    with options(e, train_batch=batch, train_seed=seed):
        for what, w in (("ones", np.ones(n, np.uint32)), ("random", rand), ("heavy", heavy), ("null", None)):
            for t0, mirror in ((0, True), (12345678901, False)):
                want = tw.draw(n, w, seed, t0, steps, batch, tw.MIRROR if mirror else 0)
                got = e.train_draw(n, steps, weights=w, t0=t0, batch=batch, mirror=mirror)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, t0)
                assert mirror == bool(got[1].any())
        if n > 1:
            assert len(set(tw.draw(n, rand, seed, 0, steps, batch)[0].tolist())) > 1
        # device pointers in and out; epoch_by_weight does not change a draw
        want = tw.draw(n, rand, seed, 5, steps, batch, tw.MIRROR)
        d_w = torch.from_numpy(rand.view(np.int32)).cuda()
        out = (torch.full((steps * batch,), -1, dtype=torch.int64, device="cuda"), torch.full((steps * batch,), 255, dtype=torch.uint8, device="cuda"))
        e.train_draw(n, steps, weights=d_w, t0=5, batch=batch, mirror=True, epoch_by_weight=True, out=out)
        assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1])
        # mirror_out may be NULL
        idx = np.full(steps * batch, -1, np.int64)
        e._check(e._lib.az_net_train_draw(e._h, n, None, 2, 5, steps, idx.ctypes.data, None))
        assert np.array_equal(idx, tw.draw(n, None, seed, 5, steps, batch)[0])


# ---- 6 .. 9. the trainer entry ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(tengine):
    """The shared set of 256 tuples, the start model (slot 8) and az_net_train's result on it at batch 32, 2 epochs, seed 1234."""
    states, boards, pis, vs = make_set(256, 77)
    tengine.net_init_random(8, seed=3)
    cfg = dict(train_epochs=2, train_batch=32, train_seed=1234)
    with options(tengine, **cfg):
        hist = tengine.train(8, 9, boards, pis, vs)
    return {"states": states, "boards": boards, "pis": pis, "vs": vs, "cfg": cfg, "hist": hist, "params": tengine.net_get_params(9)}


def test_unweighted_is_az_net_train(tengine, base):
    """weights NULL, flags 0, from boards and from the matching states, host and device memory: the parameters and the history of
    az_net_train on the same arrays, bit for bit; again with "train_graph" 0."""
    e = tengine
    for graph in (1, 0):
        with options(e, train_graph=graph, **base["cfg"]):
            for src in ("boards", "states"):
                hist = e.train_samples(8, 10, base["pis"], base["vs"], **{src: base[src]})
                assert np.array_equal(e.net_get_params(10), base["params"]), (graph, src)
                assert hist == base["hist"], (graph, src)
            dev = {k: torch.from_numpy(base[k].view(np.int64) if k == "states" else base[k]).cuda() for k in ("states", "pis", "vs")}
            e.train_samples(8, 10, dev["pis"], dev["vs"], states=dev["states"], weights=torch.ones(256, dtype=torch.int32, device="cuda"))
            assert np.array_equal(e.net_get_params(10), base["params"]), graph


def test_weighted_is_the_expansion(tengine, base):
    """Weights 0 .. 5 under AZ_TRAIN_EPOCH_BY_WEIGHT: az_net_train on the set with tuple i repeated w_i times in place."""
    e = tengine
    rng = np.random.default_rng(5)
    n = 120
    w = rng.integers(0, 6, n).astype(np.uint32)
    w[:3], w[-2:] = 0, 0
    assert 250 < w.sum() < 400
    rep = np.repeat(np.arange(n), w)
    with options(e, **base["cfg"]):
        want_hist = e.train(8, 9, base["boards"][rep], base["pis"][rep], base["vs"][rep])
        want = e.net_get_params(9)
        for src in ("states", "boards"):
            hist = e.train_samples(8, 10, base["pis"][:n], base["vs"][:n], weights=w, epoch_by_weight=True, **{src: base[src][:n]})
            assert np.array_equal(e.net_get_params(10), want) and hist == want_hist, src
        assert len(want_hist) == 2 and not np.array_equal(want, base["params"])


@pytest.mark.parametrize("case", ["mirror", "large_weights", "mirror_and_weights"])
def test_replay_through_the_step_entry(tengine, base, case):
    """az_net_train_begin / _step / _end by hand on the twin's rows, mirror bits and the documented mask seeds: AZ_TRAIN_MIRROR alone, and
    weights that include 2^31 without AZ_TRAIN_EPOCH_BY_WEIGHT (an epoch stays n / batch steps)."""
    e, n, cfg = tengine, 256, base["cfg"]
    batch, epochs, seed = cfg["train_batch"], cfg["train_epochs"], cfg["train_seed"]
    rng = np.random.default_rng(11)
    w = None
    if case != "mirror":
        w = rng.integers(0, 4, n).astype(np.uint32)
        w[[7, 200]] = 1 << 31
        w[13] = 0xFFFFFFFF
    flags = 0 if case == "large_weights" else tw.MIRROR
    steps = tw.epoch_steps(n, w, batch, flags)
    assert steps == n // batch
    idx, mir = tw.draw(n, w, seed, 0, epochs * steps, batch, flags)
    if w is not None:
        assert set(idx.tolist()) >= {7, 13, 200}
    with options(e, **cfg):
        src = "states" if case != "mirror_and_weights" else "boards"
        hist = e.train_samples(8, 10, base["pis"], base["vs"], weights=w, mirror=bool(flags), **{src: base[src]})
        got = e.net_get_params(10)
        e.train_begin(8)
        losses = []
        for t in range(epochs * steps):
            rows, m = idx[t * batch:(t + 1) * batch], mir[t * batch:(t + 1) * batch]
            b, p = tw.mirror_rows(base["boards"][rows], base["pis"][rows], m)
            losses.append(e.train_step(b, p, base["vs"][rows], mask_seed=tw.mask_seed(seed, t), apply=True)[0])
        e.train_end(11)
    assert np.array_equal(got, e.net_get_params(11))
    assert bool(mir.any()) == bool(flags) and not np.array_equal(got, base["params"])
    for ep in range(epochs):                                      # the history is the per-epoch mean of the step losses
        mean = np.mean(np.array(losses[ep * steps:(ep + 1) * steps], np.float64), axis=0)
        assert np.allclose(hist[ep], mean, rtol=1e-6, atol=0)


def test_merged_and_weighted_is_the_raw_window(tengine, base):
    """A raw set whose copies of a position carry the same pi and z (dyadic values: the fixed-point mean returns them exactly), group
    after group in first-occurrence order: az_samples_merge, then az_net_train_samples with the counts under AZ_TRAIN_EPOCH_BY_WEIGHT,
    is az_net_train on the raw set."""
    e = tengine
    rng = np.random.default_rng(21)
    m = 90
    k = rng.integers(1, 6, m)
    k[0] = 40                                                      # one heavy group, as the empty board is
    pis = rng.multinomial(64, np.ones(7) / 7, m).astype(np.float32) / 64
    vs = rng.choice([-1.0, 1.0, 0.5], m).astype(np.float32)
    states = base["states"][:m]
    assert len({tuple(s) for s in states.tolist()}) == m
    rep = np.repeat(np.arange(m), k)
    with options(e, **base["cfg"]):
        want_hist = e.train(8, 9, tw.states_to_boards(states[rep]), pis[rep], vs[rep])
        want = e.net_get_params(9)
        merged = e.merge_samples(pis[rep], vs[rep], states=states[rep])
        assert merged["count"] == m and np.array_equal(merged["counts"], k.astype(np.uint32)) and np.array_equal(merged["states"], states)
        assert fg.same_rows(merged["pis"], pis) and fg.same_rows(merged["zs"], vs)
        hist = e.train_samples(8, 10, merged["pis"], merged["zs"], states=merged["states"], weights=merged["counts"], epoch_by_weight=True)
    assert np.array_equal(e.net_get_params(10), want) and hist == want_hist


# ---- 10. the refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(tengine, engine_mod, base):
    e, em, n = tengine, engine_mod, 64
    states, boards, pis, vs = (base[k][:n].copy() for k in ("states", "boards", "pis", "vs"))
    marker = np.full(e.net_param_count(), 0.25, np.float32)
    e.net_set_params(12, marker)
    ones = np.ones(n, np.uint32)

    def samples_refused(n=n, states=states, boards=None, pis=pis, vs=vs, weights=None, flags=0, null_samples=False):
        s = em.az_samples(n, n, em._as_ptr(states), em._as_ptr(boards), em._as_ptr(pis), em._as_ptr(vs), None, None)
        st = e._lib.az_net_train_samples(e._h, 8, 12, None if null_samples else em.C.byref(s), em._as_ptr(weights), flags)
        assert st == BAD, st
        assert np.array_equal(e.net_get_params(12), marker)

    def draw_refused(n=n, weights=None, flags=0, steps=2, null_idx=False):
        idx, mir = np.full(2 * 64, -1, np.int64), np.full(2 * 64, 255, np.uint8)
        st = e._lib.az_net_train_draw(e._h, n, em._as_ptr(weights), flags, 0, steps, None if null_idx else idx.ctypes.data, mir.ctypes.data)
        assert st == BAD and (idx == -1).all() and (mir == 255).all(), st

    def bad_state(i, v):
        s = states.copy()
        s[i] = v
        return s
    with options(e, train_epochs=1):
        for refused in (samples_refused, draw_refused):
            refused(n=0)
            refused(n=-3)
            refused(weights=np.zeros(n, np.uint32))                      # W = 0
            refused(flags=4)
            refused(flags=-1)
        draw_refused(n=1 << 31)
        draw_refused(steps=0)
        draw_refused(null_idx=True)
        samples_refused(null_samples=True)
        samples_refused(pis=None)
        samples_refused(vs=None)
        samples_refused(states=None, boards=None)
        samples_refused(states=bad_state(5, (1, 1)))                     # overlapping stones
        samples_refused(states=bad_state((63, 1), states[63, 1] | np.uint64(1 << (3 * 7 + 6))), weights=ones)      # a bit at col * 7 + 6
        samples_refused(states=bad_state((0, 0), np.uint64(1 << 49)))    # a bit outside the seven columns
        e.train_begin(8)                                                 # an open training session
        try:
            samples_refused()
            draw_refused()
        finally:
            e.train_end(13)
        e.selfplay_begin(4, 10, 8, seed=1)                               # an open self-play session
        try:
            samples_refused()
            draw_refused()
        finally:
            e.selfplay_end()
        # the same calls go through once nothing is open; a weight of 0 beside others is legal
        w = ones.copy()
        w[::2] = 0
        e.train_samples(8, 12, pis, vs, states=states, weights=w)
        assert not np.array_equal(e.net_get_params(12), marker)
        assert set(e.train_draw(n, 2, weights=w, batch=64)[0].tolist()) <= set(range(1, n, 2))


# ---- 11. purity ------------------------------------------------------------------------------------------------------------------------------
def test_draw_is_pure(tengine, base):
    e = tengine
    rng = np.random.default_rng(3)
    w = rng.integers(0, 9, 5000).astype(np.uint32)
    with options(e, **base["cfg"]):
        models = {i: e.net_get_params(i) for i in (8, 9)}
        e.reset_stats()
        zero = e.stats()
        a = e.train_draw(5000, 4, weights=w, t0=3, batch=32, mirror=True)
        b = e.train_draw(5000, 4, weights=w, t0=3, batch=32, mirror=True)
        st = e.stats()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert {k: v for k, v in st.items() if k != "device_ms"} == {k: v for k, v in zero.items() if k != "device_ms"}
        for i, p in models.items():
            assert np.array_equal(e.net_get_params(i), p), i
        # the options are where they were: az_net_train still gives the bits it gave before the draws
        hist = e.train(8, 10, base["boards"], base["pis"], base["vs"])
        assert np.array_equal(e.net_get_params(10), base["params"]) and hist == base["hist"]


# ---- 12. both Coaches --------------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_coach_agree(engine_mod, tmp_path):
    """Two iterations at a tiny configuration with merge_positions, merge_canonical and merge_weighted on both hosts: the same report,
    byte-identical files; the last candidate is what merge_samples + train_samples give by hand on the window with the same seed."""
    from alphazero_rs_amd import coach as cm
    seed, iters = 11, 2
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp")}
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=C)
    try:
        e.net_init_random(0, 3)
        e.set_option("train_epochs", 1)
        coach = cm.Coach.setup(e, dirs["py"], 1000000, 0.55, 15, 3, 100000, 1, 64, 8, iters, 16, 25, 1, 1000, 1, log=lambda m: None)
        coach.merge_positions = coach.merge_canonical = coach.merge_weighted = True
        rep = coach.learn(seed=seed)
        window = [np.concatenate([h[i] for h in coach.history]) for i in range(3)]
        # the candidate of the last iteration by hand
        last = rep[-1]
        if last["model_id"] == 0:
            e.net_init_random(20, 3)
        else:
            e.net_load(20, os.path.join(dirs["py"], "%d.aznet" % last["model_id"]))
        merged = e.merge_samples(window[1], window[2], boards=window[0], canonical=True)
        perm = cm.shuffle_permutation(merged["count"], seed, last["iteration"])
        e.set_option("train_seed", seed + last["iteration"])
        e.train_samples(20, 21, merged["pis"][perm], merged["zs"][perm], states=merged["states"][perm], weights=merged["counts"][perm], mirror=True)
        e.net_load(22, os.path.join(dirs["py"], "%d.aznet" % (last["model_id"] + 1)))
        assert np.array_equal(e.net_get_params(21), e.net_get_params(22))
        assert last["samples"] == merged["count"] and last["samples_weight"] == int(merged["counts"].sum()) == len(window[2])
    finally:
        e.close()
    exe = os.path.join(tmp_path, "test_coach_weighted")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_weighted.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, dirs["cpp"], str(C), str(seed), str(iters), "1"], check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    crep = json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    assert len(rep) == len(crep) == iters
    for r, c in zip(rep, crep):
        for k in fg.REPORT_KEYS + ("samples_raw", "samples_weight"):
            assert r[k] == c[k], k
        assert r["samples"] < r["samples_raw"] == r["samples_weight"]
    fg.compare_directories(dirs["py"], dirs["cpp"], required=("0.examples", "1.examples", "1.aznet"))
