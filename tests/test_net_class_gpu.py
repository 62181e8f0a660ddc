"""GPU tests of the numerics class of a MODEL (az_net_set_class / az_net_get_class) and of the fp8 skinny GEMM (k_gemm_skinny_f8).

The two reference engines of this file run the parent's code paths -- a plain bf16 engine and an engine with "net_fp8" = 1 on which
nobody calls az_net_set_class -- and every comparison with them is bit for bit: no tolerance is involved anywhere except where the
emulation's exp / tanh meet the device's (the 1e-6 of tests/test_fp8_gpu.py::test_exact_integer_data_bit_for_bit, kept as it is).
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import net_ref_fp8 as r8
from net_ref import random_params
from test_fp8_gpu import boards_of, conv3_codes, exact_params, fp8_scales
from test_net_gpu import _check_move_record, _flatten_log, random_states

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = 512
AZ_ERR_BAD_ARGUMENT = 1
ENGINE, BF16, FP8 = -1, 0, 1


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def skinny_launches(e):
    f = e._lib.az_diag_fp8_skinny_launches
    f.restype = C.c_longlong
    f.argtypes = [C.c_void_p]
    n = int(f(e._h))
    assert n >= 0
    return n


@pytest.fixture(scope="module")
def refs(engine_mod):
    """(bf16 engine, "net_fp8" = 1 engine) at C = 512: the parent's two code paths."""
    a = engine_mod.Engine(device=0, max_batch=8192, net_channels=CH)
    b = engine_mod.Engine(device=0, max_batch=8192, net_channels=CH)
    b.set_option("net_fp8", 1)
    yield a, b
    a.close()
    b.close()


def test_one_engine_three_classes(engine_mod, oracle, refs):
    """The same parameters in ids 0, 1, 2 set to BF16, FP8 and ENGINE: id 0 is the bf16 engine bit for bit, id 1 the net_fp8 engine,
    id 2 follows az_set_option("net_fp8") both ways -- at one row, a ragged skinny batch, both ring families and a big batch."""
    ref16, ref8 = refs
    params = random_params(CH, seed=31)
    ref16.net_set_params(0, params)
    ref8.net_set_params(0, params)
    e = engine_mod.Engine(device=0, max_batch=8192, net_channels=CH)
    try:
        for mid in (0, 1, 2):
            e.net_set_params(mid, params)
            assert e.net_class(mid) == (ENGINE, 0)
        e.net_set_class(0, engine_mod.NET_CLASS_BF16)
        e.net_set_class(1, engine_mod.NET_CLASS_FP8)
        e.net_set_class(2, engine_mod.NET_CLASS_ENGINE)
        assert [e.net_class(m) for m in (0, 1, 2)] == [(BF16, 0), (FP8, 1), (ENGINE, 0)]
        states = random_states(oracle, 3100, seed=5)
        for n in (1, 13, 240, 700, 3100):
            b, f = ref16.predict_states(states[:n], 0), ref8.predict_states(states[:n], 0)
            assert not np.array_equal(b[0], f[0])
            for opt in (0, 1, 0):
                e.set_option("net_fp8", opt)
                assert [e.net_class(m) for m in (0, 1, 2)] == [(BF16, 0), (FP8, 1), (ENGINE, opt)]
                assert same(e.predict_states(states[:n], 0), b), (n, opt)
                assert same(e.predict_states(states[:n], 1), f), (n, opt)
                assert same(e.predict_states(states[:n], 2), f if opt else b), (n, opt)
        # the class survives uploads into the id: other weights, then these again; and a training session ending in the id
        e.net_set_params(1, random_params(CH, seed=32))
        assert e.net_class(1) == (FP8, 1) and not same(e.predict_states(states[:13], 1), ref8.predict_states(states[:13], 0))
        e.net_set_params(1, params)
        assert e.net_class(1) == (FP8, 1) and same(e.predict_states(states[:13], 1), ref8.predict_states(states[:13], 0))
        e.train_begin(0)
        e.train_end(1)
        assert e.net_class(1) == (FP8, 1) and same(e.predict_states(states[:240], 1), ref8.predict_states(states[:240], 0))
        e.net_init_random(1, seed=3)
        assert e.net_class(1) == (FP8, 1)
    finally:
        e.close()


@pytest.mark.parametrize("channels", [512, 256])
def test_fp8_skinny_runs_and_is_bit_identical(engine_mod, oracle, channels):
    """An FP8 model of a diagnostic engine at 1, 12, 16, 17 and 32 boards: "narrow_rows" = 32 takes the batch on k_gemm_skinny_f8 (the
    launch counter rises: one launch for conv3, one for conv4), "narrow_rows" = 0 leaves it on the ring (the counter stays put), and
    conv3's e4m3 codes, pi and v are equal byte for byte."""
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=channels, diag=True)
    try:
        e.net_set_params(0, random_params(channels, seed=channels + 1))
        e.net_set_class(0, engine_mod.NET_CLASS_FP8)
        states = random_states(oracle, 32, seed=61)
        for n in (1, 12, 16, 17, 32):
            e.set_option("narrow_rows", 0)
            c0 = skinny_launches(e)
            ring = e.predict_states(states[:n], 0)
            ring_codes = conv3_codes(e, n, channels)
            assert skinny_launches(e) == c0, n
            e.set_option("narrow_rows", 32)
            sk = e.predict_states(states[:n], 0)
            sk_codes = conv3_codes(e, n, channels)
            c1 = skinny_launches(e)
            print(f"C {channels} n {n}: skinny launches {c0} -> {c1}; codes that differ {int((ring_codes != sk_codes).sum())}; "
                  f"max |dpi| {np.abs(ring[0] - sk[0]).max():.3e} max |dv| {np.abs(ring[1] - sk[1]).max():.3e}")
            assert c1 == c0 + 2, (n, c0, c1)
            assert (ring_codes != 0).mean() > 0.05
            assert np.array_equal(ring_codes, sk_codes), (n, int((ring_codes != sk_codes).sum()))
            assert same(ring, sk), n
        # one board more than the line: the ring takes it (both kernels are launched, the device decides), the same bits again
        more = random_states(oracle, 70, seed=62)
        e.set_option("narrow_rows", 0)
        ring = e.predict_states(more, 0)
        e.set_option("narrow_rows", 32)
        for n in (33, 64, 65, 70):
            assert same(e.predict_states(more[:n], 0), (ring[0][:n], ring[1][:n])), n
    finally:
        e.close()


def test_fp8_skinny_exact_integer_data(engine_mod, oracle):
    """The exact-integer net of tests/test_fp8_gpu.py at C = 256 through the skinny path: conv3's e4m3 output equals the emulation
    (tests/net_ref_fp8.py) bit for bit -- a wrong lane -> chunk pairing, swizzle, tap offset, stage offset, scale or conversion changes
    integers -- pi and v equal the ring's bit for bit and the emulation's to the 1e-6 that test allows for exp / tanh."""
    ch = 256
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=ch, diag=True)
    try:
        params = exact_params(ch, seed=5)
        e.net_set_params(0, params)
        e.net_set_class(0, engine_mod.NET_CLASS_FP8)
        sa2, sa3 = fp8_scales(e, 0)
        states = random_states(oracle, 32, seed=21)
        for n in (32, 17, 1):
            boards = boards_of(oracle, states[:n])
            e.set_option("narrow_rows", 32)
            c0 = skinny_launches(e)
            pi, v = e.predict_states(states[:n], 0)
            codes = conv3_codes(e, n, ch)
            assert skinny_launches(e) == c0 + 2
            epi, ev, info = r8.forward_fp8(params, boards, ch, sa2, sa3, details=True)
            print(f"exact n {n}: distinct codes {np.unique(codes).size}; codes that differ {int((codes != info['act3_codes']).sum())}; "
                  f"max |dpi| {np.abs(pi - epi).max():.3e} max |dv| {np.abs(v - ev).max():.3e}")
            if n == 32:
                assert np.unique(codes).size > 16 and (codes != 0).mean() > 0.1      # the data exercise the format
            assert np.array_equal(codes, info["act3_codes"]), int((codes != info["act3_codes"]).sum())
            assert np.abs(pi - epi).max() <= 1e-6 and np.abs(v - ev).max() <= 1e-6
            e.set_option("narrow_rows", 0)
            assert same(e.predict_states(states[:n], 0), (pi, v)), n
    finally:
        e.close()


def _arena_rows_equal(logs, which, ref_engine, ref_id):
    """Every recorded row of seat `which` is what ref_engine.predict_states returns for its state, bit for bit."""
    cnt, states, pis, vs = logs[which]
    sel = np.arange(states.shape[1])[None, :] < cnt[:, None]
    st, pi, v = states[sel], pis[sel], vs[sel]
    assert st.shape[0] == int(cnt.sum()) > 0
    rpi, rv = ref_engine.predict_states(st, ref_id)
    bad = np.flatnonzero(~((rpi == pi).all(axis=1) & (rv == v)))
    assert bad.size == 0, (which, bad.size, st.shape[0])
    return st, pi, v


def _mixed_arena(e, oracle, new_id, old_id, num, sims, seed):
    cap = 22 * (sims + 1) + 8
    wld, res = e.arena(num, sims, new_model_id=new_id, old_model_id=old_id, seed=seed, record_evals=cap)
    assert int(wld.sum()) == num
    logs = [e.arena_get_evals(w, num, cap) for w in (0, 1)]
    assert max(int(l[0].max()) for l in logs) <= cap
    sel = list(range(num))                                      # every game: none is left out
    rn, ro = (_flatten_log(*logs[w], sel) for w in (0, 1))
    owld, ores, bad = oracle.arena_ex(num, sims, first_game=0, n_games=num, net_kind=oracle.NET_REPLAY, seed=seed, threads=16, replay_new=rn, replay_old=ro)
    assert not bad.any(), np.flatnonzero(bad)[:5]
    assert np.array_equal(ores, res) and owld.tolist() == wld.tolist()
    glen, gmoves = e.arena_get_moves(num)
    _check_move_record(oracle, glen, gmoves, res)
    return logs


def test_mixed_arena_fp8_against_bf16(engine_mod, oracle, refs):
    """az_arena with new = FP8 and old = BF16 on one engine, two different conv nets, 256 games at 100 simulations: every game replays
    on the oracle, every recorded row of seat new is the net_fp8 engine's, every row of seat old the bf16 engine's.  Then the SAME
    parameters in both seats: the two seats' rows of the same states differ somewhere (the classes really are two), replay still clean."""
    ref16, ref8 = refs
    e = engine_mod.Engine(device=0, max_batch=8192, net_channels=CH)
    try:
        pa, pb = random_params(CH, seed=41), random_params(CH, seed=42)
        for eng in (e, ref16, ref8):
            eng.net_set_params(22, pa)
            eng.net_set_params(23, pb)
        e.net_set_class(23, engine_mod.NET_CLASS_FP8)
        e.net_set_class(22, engine_mod.NET_CLASS_BF16)
        num, sims = 256, 100
        logs = _mixed_arena(e, oracle, 23, 22, num, sims, seed=9)
        _arena_rows_equal(logs, 0, ref8, 23)
        _arena_rows_equal(logs, 1, ref16, 22)
        # the same net against its own fp8 copy
        e.net_set_params(24, pb)
        e.net_set_class(24, engine_mod.NET_CLASS_BF16)
        logs = _mixed_arena(e, oracle, 23, 24, num, sims, seed=10)
        sn, pn, vn = _arena_rows_equal(logs, 0, ref8, 23)
        so, po, vo = _arena_rows_equal(logs, 1, ref16, 23)
        rows_old = {(int(a), int(b)): (po[i].tobytes(), vo[i].tobytes()) for i, (a, b) in enumerate(so[:20000])}
        shared = differ = 0
        for i, (a, b) in enumerate(sn[:20000]):
            r = rows_old.get((int(a), int(b)))
            if r is not None:
                shared += 1
                differ += r != (pn[i].tobytes(), vn[i].tobytes())
        print("same net, two classes: states both seats evaluated", shared, "rows that differ", differ)
        assert shared > 0 and differ > 0
    finally:
        e.close()


def test_class_change_retags_one_model_and_its_graphs(engine_mod, oracle):
    """A persistent evaluation cache: flipping model 0's class BF16 -> FP8 -> BF16 gives the other class's games and then the first
    ones again (no stale row is served), each equal to the reference engine's of that class; model 1's tag is untouched by all of it
    (a repeat of its self-play is answered by the cache), also by a set_class that leaves its effective class alone; while
    az_set_option("net_fp8") retags it.  Then 1-tree searches with the search graph on, flipping back and forth: the right class
    each time."""
    C_ = 128
    e = engine_mod.Engine(device=0, max_batch=512, net_channels=C_)
    r16 = engine_mod.Engine(device=0, max_batch=512, net_channels=C_)
    r8e = engine_mod.Engine(device=0, max_batch=512, net_channels=C_)
    try:
        r8e.set_option("net_fp8", 1)
        for eng in (e, r16, r8e):
            eng.net_init_random(0, seed=5)
            eng.net_init_random(1, seed=6)
        e.set_option("eval_cache_log2", 22)
        e.set_option("eval_cache_persist", 1)
        play = lambda eng, mid: eng.selfplay(n_games=64, num_sims=50, model_id=mid, seed=3)
        want = {BF16: play(r16, 0), FP8: play(r8e, 0)}
        assert not (want[BF16]["pis"].shape == want[FP8]["pis"].shape and np.array_equal(want[BF16]["pis"], want[FP8]["pis"]))
        e.reset_stats()
        first1 = play(e, 1)
        cold = e.stats()["leaf_rows_executed"]
        assert cold > 1000
        for cls in (BF16, FP8, BF16, FP8, ENGINE):
            e.net_set_class(0, cls)
            got = play(e, 0)
            for key in ("moves", "game_len", "pis", "zs", "boards"):
                assert np.array_equal(got[key], want[BF16 if cls == ENGINE else cls][key]), (cls, key)
        e.net_set_class(1, engine_mod.NET_CLASS_BF16)             # stored class changes, effective class does not: the tag stays
        assert e.net_class(1) == (BF16, 0)
        e.reset_stats()
        again1 = play(e, 1)
        st = e.stats()
        print("model 1 repeat after model 0's flips: rows executed", st["leaf_rows_executed"], "of", cold, "cache hits", st["eval_cache_hits"])
        for key in ("moves", "game_len", "pis", "zs"):
            assert np.array_equal(again1[key], first1[key]), key
        assert st["eval_cache_hits"] > 0 and st["leaf_rows_executed"] * 20 < cold
        e.net_set_class(1, engine_mod.NET_CLASS_FP8)              # its own flip: nothing of the bf16 rows may be served
        e.reset_stats()
        fp1 = play(e, 1)
        st = e.stats()
        ref1 = play(r8e, 1)
        for key in ("moves", "game_len", "pis", "zs"):
            assert np.array_equal(fp1[key], ref1[key]), key
        assert st["leaf_rows_executed"] * 2 > cold
        # ---- a cached search graph: 1-tree calls, 100 simulations, the class flipped between calls
        root = random_states(oracle, 1, seed=4)
        def search(eng, tree):
            tree.reset(root)
            return tree.get_action_prob(root, 0.0, seed=7)
        trees = {k: eng.tree_create(1, 100000, 100, 1000, 0, 1) for k, eng in (("e", e), (BF16, r16), (FP8, r8e))}
        try:
            wantt = {k: search(eng, trees[k]) for k, eng in ((BF16, r16), (FP8, r8e))}
            assert not np.array_equal(wantt[BF16][2], wantt[FP8][2])
            for cls in (BF16, FP8, FP8, BF16, FP8, BF16):
                e.net_set_class(0, cls)
                got = search(e, trees["e"])
                for a, b in zip(got, wantt[cls]):
                    assert np.array_equal(a, b), cls
        finally:
            for t in trees.values():
                t.close()
    finally:
        for eng in (e, r16, r8e):
            eng.close()


def test_class_refusals_and_lifetime(engine_mod, oracle):
    """Each refusal is AZ_ERR_BAD_ARGUMENT with a message and leaves the state as it was: a stub model, an unknown id, FP8 with
    "conv2_table" = 0, "conv2_table" = 0 with an FP8 model present, any change during an open session.  az_net_free drops the class."""
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    try:
        e.net_init_random(0, seed=5)
        e.net_set_kind(5, engine_mod.NET_STUB, 0)
        states = random_states(oracle, 40, seed=9)
        bf = e.predict_states(states, 0)

        def refused(fn, *args):
            with pytest.raises(engine_mod.AzError) as ei:
                fn(*args)
            assert ei.value.status == AZ_ERR_BAD_ARGUMENT, args
            assert len(e._lib.az_last_error(e._h)) > 0

        refused(e.net_set_class, 5, engine_mod.NET_CLASS_FP8)                  # a stub model
        refused(e.net_class, 5)
        refused(e.net_set_class, 99, engine_mod.NET_CLASS_FP8)                 # an unknown id ...
        refused(e.net_class, 99)
        with pytest.raises(engine_mod.AzError):                                # ... which the call did not create
            e.net_get_params(99)
        refused(e.net_set_class, 0, 7)                                         # not a class
        e.set_option("conv2_table", 0)
        refused(e.net_set_class, 0, engine_mod.NET_CLASS_FP8)                  # FP8 needs the table
        assert e.net_class(0) == (ENGINE, 0)
        e.net_set_class(0, engine_mod.NET_CLASS_BF16)                          # bf16 does not
        e.net_set_class(0, engine_mod.NET_CLASS_ENGINE)
        e.set_option("conv2_table", 1)
        assert same(e.predict_states(states, 0), bf)
        e.net_set_class(0, engine_mod.NET_CLASS_FP8)
        f8 = e.predict_states(states, 0)
        assert not np.array_equal(f8[0], bf[0])
        refused(e.set_option, "conv2_table", 0)                                # an FP8 model is present
        assert "conv2_table" in e._lib.az_last_error(e._h).decode()
        assert e.net_class(0) == (FP8, 1) and same(e.predict_states(states, 0), f8)
        e.selfplay_begin(n_games=8, concurrent=4, num_sims=25, model_id=0, seed=1)
        try:
            refused(e.net_set_class, 0, engine_mod.NET_CLASS_BF16)             # an open session
            refused(e.net_set_class, 0, engine_mod.NET_CLASS_ENGINE)
            assert e.net_class(0) == (FP8, 1)
        finally:
            e.selfplay_end()
        assert same(e.predict_states(states, 0), f8)
        e.net_free(0)
        refused(e.net_class, 0)
        e.net_init_random(0, seed=5)
        assert e.net_class(0) == (ENGINE, 0) and same(e.predict_states(states, 0), bf)
        e.set_option("conv2_table", 0)                                         # nothing is fp8 any more
        e.set_option("conv2_table", 1)
    finally:
        e.close()


COACH_ARGS = (1000000, 0.55, 15, 3, 100000, 1, 64, 16, 2, 48, 25, 1, 1000, 1)       # the configuration of tests/cpp/test_coach.cpp


def _same_files(da, db):
    files = sorted(os.listdir(da))
    assert files == sorted(os.listdir(db)) and "0.examples" in files and "1.examples" in files and "1.aznet" in files
    for f in files:
        with open(os.path.join(da, f), "rb") as x, open(os.path.join(db, f), "rb") as y:
            assert x.read() == y.read(), f
    return files


def test_coach_selfplay_class(engine_mod, tmp_path):
    """Coach.selfplay_class = FP8 in both hosts: byte-identical files; iteration 0's episodes are az_selfplay of an FP8-pinned model
    (and not the bf16 run's); the arena's recorded rows are bf16 rows.  The knob at its default: no class call at all, and the files
    of the Python host, of the C++ host with the knob absent and of the C++ host with the knob set to ENGINE are the same."""
    from alphazero_rs_amd.coach import Coach, load_examples
    Cn, seed = 128, 11
    cap = 22 * 26 + 8
    dirs = {k: os.path.join(tmp_path, k) for k in ("py_fp8", "cpp_fp8", "py_default", "cpp_absent", "cpp_engine")}

    def run_python(directory, cls):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=Cn)
        calls, arenas = [], []
        try:
            e.net_init_random(0, 3)
            e.set_option("train_epochs", 2)
            set_class, arena = e.net_set_class, e.arena
            e.net_set_class = lambda mid, c: (calls.append((mid, int(c))), set_class(mid, c))[1]

            def recording_arena(*a, **k):
                out = arena(*a, record_evals=cap, **k)
                arenas.append((k["new_model_id"], k["old_model_id"], [e.arena_get_evals(w, 16, cap) for w in (0, 1)],
                               [e.net_class(k["new_model_id"]), e.net_class(k["old_model_id"])]))
                return out
            if cls is not None:
                e.arena = recording_arena
            coach = Coach.setup(e, directory, *COACH_ARGS, log=lambda m: None)
            if cls is not None:
                coach.selfplay_class = cls
            return coach.learn(seed=seed), calls, arenas
        finally:
            e.close()

    exe = os.path.join(tmp_path, "test_coach_class")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_coach_class.cpp"), "-o", exe, "-L", libdir, "-laz_engine",
                           f"-Wl,-rpath,{libdir}"])

    def run_cpp(directory, cls):
        out = subprocess.run([exe, directory, str(Cn), str(seed), cls], check=True, stdout=subprocess.PIPE, text=True, timeout=900).stdout
        lines = out.strip().splitlines()
        return json.loads([l for l in lines if l.startswith("[")][-1]), json.loads([l for l in lines if l.startswith("{")][-1])

    rep, calls, arenas = run_python(dirs["py_fp8"], engine_mod.NET_CLASS_FP8)
    crep, live = run_cpp(dirs["cpp_fp8"], "1")
    assert len(rep) == len(crep) == 2
    for a, b in zip(rep, crep):
        for k in ("iteration", "samples", "nwins", "pwins", "draws", "accepted", "model_id"):
            assert a[k] == b[k], (k, a, b)
        assert np.allclose(np.array(a["losses"]).reshape(-1), b["losses"], rtol=1e-6)
    _same_files(dirs["py_fp8"], dirs["cpp_fp8"])
    assert live["live_class"] == [BF16, 0]              # the live model left the last gate pinned to bf16; the next iteration pins it to fp8 again
    # per iteration: the playing model to FP8, then both arena models to BF16
    m0, m1 = rep[0]["model_id"], rep[1]["model_id"]
    assert calls == [(m0, FP8), (m0 + 1, BF16), (m0, BF16), (m1, FP8), (m1 + 1, BF16), (m1, BF16)], calls
    # iteration 0's episodes: an FP8-pinned model's az_selfplay
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=Cn)
    r16 = engine_mod.Engine(device=0, max_batch=256, net_channels=Cn)
    try:
        e.net_init_random(0, 3)
        e.net_set_class(0, engine_mod.NET_CLASS_FP8)
        sp = e.selfplay(n_games=48, num_sims=25, model_id=0, seed=seed, first_game_id=0, concurrent=48, temp_threshold=15, max_depth=1000,
                        cpuct=1, reserve=1000000, symmetries=True)
        boards, pis, vs = load_examples(os.path.join(dirs["py_fp8"], "0.examples"))[0]
        assert np.array_equal(sp["boards"], boards) and np.array_equal(sp["pis"], pis) and np.array_equal(sp["zs"], vs)
        # the gate: both models bf16 while the arena ran, and every recorded row is the bf16 row of its state
        assert len(arenas) == 2
        for new_id, old_id, logs, classes in arenas:
            assert classes == [(BF16, 0), (BF16, 0)]
            for which, mid in ((0, new_id), (1, old_id)):
                r16.net_load(mid, os.path.join(dirs["py_fp8"], f"{mid}.aznet"))
                st, _, _ = _arena_rows_equal(logs, which, r16, mid)
                e.net_load(7, os.path.join(dirs["py_fp8"], f"{mid}.aznet"))
                e.net_set_class(7, engine_mod.NET_CLASS_FP8)
                assert not same(e.predict_states(st[:256], 7), r16.predict_states(st[:256], mid))      # fp8 rows would have been others
    finally:
        e.close()
        r16.close()
    # the default: today's runs
    rep_d, calls_d, _ = run_python(dirs["py_default"], None)
    assert calls_d == []
    run_cpp(dirs["cpp_absent"], "absent")
    run_cpp(dirs["cpp_engine"], "-1")
    _same_files(dirs["py_default"], dirs["cpp_absent"])
    _same_files(dirs["py_default"], dirs["cpp_engine"])
    b0 = load_examples(os.path.join(dirs["py_default"], "0.examples"))[0]
    assert not (b0[1].shape == pis.shape and np.array_equal(b0[1], pis))                    # the fp8 episodes are other episodes
