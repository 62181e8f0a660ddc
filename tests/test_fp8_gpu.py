"""GPU tests of the "net_fp8" numerics class (az_set_option "net_fp8" = 1: conv3 and conv4 on the e4m3 matrix path).

The class is not bit-identical to bf16 and does not claim to be; what it does claim is checked here: exact integer data come out bit
for bit (lane -> k map, tap walk, scales, conversions), random nets stay within a measured distance of the torch emulation
(tests/net_ref_fp8.py) run with the engine's own activation scales, a row depends on its state alone, searches replay on the oracle,
and switching the class never mixes cached rows.
"""
import ctypes as C

import numpy as np
import pytest

import net_ref_fp8 as r8
from net_ref import exact_params, forward_ref, layout, random_params
from test_net_gpu import (_check_move_record, _flatten_log, _replay_every_episode, assert_every_recorded_row_is_the_net, hold_a_draining_selfplay,
                          hold_an_arena_and_a_tree_search, random_states)

pytestmark = pytest.mark.gpu
CH = 512
AZ_ERR_BAD_ARGUMENT = 1


def fp8_scales(e, model_id):
    """(sa2, sa3) of a model of a diagnostic-library engine."""
    f = e._lib.az_diag_fp8_scales
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    out = np.zeros(2, np.float32)
    assert f(e._h, model_id, out.ctypes.data_as(C.c_void_p)) == 0
    return float(out[0]), float(out[1])


def conv3_codes(e, rows, channels):
    """conv3's e4m3 output of the engine's last forward: rows x [4][5][C] codes (diagnostic library's reader)."""
    f = e._lib.az_diag_read_conv3_out_fp8
    f.restype = C.c_longlong
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    out = np.empty((rows, 4, 5, channels), np.uint8)
    assert f(e._h, rows, out.ctypes.data_as(C.c_void_p)) == out.nbytes
    return out


def boards_of(oracle, states):
    return np.stack([oracle.c4_features(int(m), int(t)) for m, t in states])


@pytest.fixture(scope="module")
def fp8_diag(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=8192, net_channels=CH, diag=True)
    e.set_option("net_fp8", 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fp8_engine(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=8192, net_channels=CH)
    e.set_option("net_fp8", 1)
    yield e
    e.close()


def test_exact_integer_data_bit_for_bit(engine_mod, oracle):
    """Integer data through the whole fp8 path at C = 256 (two column tiles, two 128-channel blocks): conv3's e4m3 output equals the
    emulation bit for bit -- a wrong lane -> k pairing, tap offset, swizzle, scale or conversion changes integers -- and pi, v agree
    to 1e-6 (the layers behind conv3 are exact too; what is left is exp / tanh)."""
    ch = 256
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=ch, diag=True)
    try:
        e.set_option("net_fp8", 1)
        params = exact_params(ch, seed=5)
        e.net_set_params(0, params)
        sa2, sa3 = fp8_scales(e, 0)
        states = random_states(oracle, 150, seed=21)
        boards = boards_of(oracle, states)
        pi, v = e.predict_states(states, 0)
        codes = conv3_codes(e, len(states), ch)
        epi, ev, info = r8.forward_fp8(params, boards, ch, sa2, sa3, details=True)
        print("exact: scales", sa2, sa3, "largest scaled activations", info["max_scaled"], "distinct codes", np.unique(codes).size,
              "max |dpi|", np.abs(pi - epi).max(), "max |dv|", np.abs(v - ev).max())
        assert np.unique(codes).size > 16 and (codes != 0).mean() > 0.1          # the data exercise the format
        assert np.array_equal(codes, info["act3_codes"]), int((codes != info["act3_codes"]).sum())
        assert np.abs(pi - epi).max() <= 1e-6 and np.abs(v - ev).max() <= 1e-6
        assert 1e-3 < pi.max() < 0.999 and np.abs(v).max() < 0.999                  # nothing saturated that could hide a difference
    finally:
        e.close()


# GPU against the emulation run with the engine's own (sa2, sa3).  The emulation rounds where the engine rounds (conv1's table in the
# kernel's own summation order, conv2's f16 table terms) and sums without an order of its own; what is left is the summation inside
# v_mfma_f32_16x16x128_f8f6f4, which now and then moves an e4m3 rounding of one activation by a whole step: 2^-4 relative, against
# 2^-8 in bf16 (1e-5 .. 4e-5 of conv2's codes and 2e-4 .. 9e-4 of conv3's are one step away).  It is NOT the order of an f32
# accumulation: an f32 sum of the same exact products, sequential or in 128-product blocks, lands on the nearest code in all but
# 1.5e-6 of the elements at most (tests/test_net_layers_fp8_cpu.py), while the device, teacher-forced on bit-identical inputs, is one step off
# in 2.2e-4 .. 4.3e-4 (tests/test_net_layers_fp8_gpu.py) -- the instruction's sum of its 128 products is less accurate than f32's,
# inside the worst-case f32 bound all the same.  Nor is it inherited: conv2's codes are its table's bit for bit, and the few codes
# in which the emulation's conv2 differs (its table terms are summed in float64, the engine's in the table GEMM's f32 order before
# the f16 rounding) account for a sixth to a third of conv3's end-to-end differences, the MFMA for the rest.  Measured on the MI355X
# (random_params(512, seed = batch), batches 1 / 3 / 130 / 700): max |dpi| 2.2e-6 / 1.5e-4 / 3.0e-4 / 4.0e-4, max |dv|
# 9.7e-8 / 7.0e-4 / 1.9e-3 / 3.0e-3.  The bar is 3 x the largest value seen:
BAR_PI, BAR_V = 3 * 4.024e-4, 3 * 2.995e-3


@pytest.mark.parametrize("batch", [1, 3, 130, 700])
def test_fp8_matches_the_emulation(fp8_diag, oracle, batch):
    """The engine within the measured bar of the emulation (figures above), closer to the fp8 emulation than to the bf16 one (measured
    distance to the bf16 emulation: |dpi| 2.1e-3 .. 4.2e-3, |dv| 7.2e-3 .. 2.2e-2 -- four to a thousand times its distance to the fp8
    emulation), no farther from the textbook f32 net than the emulation is plus the bar (measured: engine 2.1e-3 .. 4.3e-3 / 7.6e-3 ..
    2.0e-2, emulation 2.1e-3 .. 4.2e-3 / 7.6e-3 .. 2.0e-2), power-of-two scales (64 and 32 or 64 on these nets), nothing saturated
    (largest scaled activations 70 .. 95 of 448)."""
    params = random_params(CH, seed=batch)
    fp8_diag.net_set_params(2, params)
    sa2, sa3 = fp8_scales(fp8_diag, 2)
    states = random_states(oracle, batch, seed=100 + batch)
    boards = boards_of(oracle, states)
    pi, v = fp8_diag.predict_states(states, 2)
    codes = conv3_codes(fp8_diag, batch, CH)
    epi, ev, info = r8.forward_fp8(params, boards, CH, sa2, sa3, details=True)
    bpi, bv = forward_ref(params, boards, CH, emulate_bf16=True)
    fpi, fv = forward_ref(params, boards, CH, emulate_bf16=False)
    d = lambda a, b: float(np.abs(a - b).max())
    print(f"fp8 batch {batch}: scales {sa2} {sa3}; gpu-emu {d(pi, epi):.3e} {d(v, ev):.3e}; gpu-bf16emu {d(pi, bpi):.3e} {d(v, bv):.3e}; "
          f"emu-bf16emu {d(epi, bpi):.3e} {d(ev, bv):.3e}; gpu-f32 {d(pi, fpi):.3e} {d(v, fv):.3e}; emu-f32 {d(epi, fpi):.3e} {d(ev, fv):.3e}; "
          f"largest scaled activations {info['max_scaled']}; largest act3 code {int((codes & 0x7F).max()):#x}; "
          f"act3 codes that differ from the emulation's {float((codes != info['act3_codes']).mean()):.2e}")
    for s in (sa2, sa3):
        assert s > 0 and np.log2(s) == int(np.log2(s)), s
    assert max(info["max_scaled"]) < 448.0 and int((codes & 0x7F).max()) < 0x7E          # no test activation saturates
    assert np.all(np.abs(pi.sum(axis=1) - 1) < 1e-5)
    assert d(pi, epi) <= BAR_PI and d(v, ev) <= BAR_V
    assert d(pi, epi) < d(pi, bpi) and d(v, ev) < d(v, bv)                               # the fp8 class, not bf16
    assert d(pi, fpi) <= d(epi, fpi) + BAR_PI and d(v, fv) <= d(ev, fv) + BAR_V


def test_the_bar_can_tell_the_classes_apart(oracle):
    """The condition on the bar above: it must stay below half of the emulated fp8-vs-bf16 gap on the same inputs (the four batches
    together, as the bar is the largest value over the four) -- otherwise a result could sit within the bar of both classes.
    Measured gap: |dpi| 4.19e-3, |dv| 2.116e-2, so the bars of 1.21e-3 / 8.99e-3 stand against 2.09e-3 / 1.058e-2."""
    gap_pi = gap_v = 0.0
    for batch in (1, 3, 130, 700):
        params = random_params(CH, seed=batch)
        boards = boards_of(oracle, random_states(oracle, batch, seed=100 + batch))
        sa2, sa3 = r8.calibrate_scales(params, boards, CH)          # 64 and 32 or 64, as the engine's calibration set gives
        epi, ev = r8.forward_fp8(params, boards, CH, sa2, sa3)
        bpi, bv = forward_ref(params, boards, CH, emulate_bf16=True)
        gap_pi, gap_v = max(gap_pi, float(np.abs(epi - bpi).max())), max(gap_v, float(np.abs(ev - bv).max()))
    print("emulated fp8-vs-bf16 gap:", gap_pi, gap_v)
    assert BAR_PI < 0.5 * gap_pi and BAR_V < 0.5 * gap_v, (gap_pi, gap_v)


def test_fp8_rows_depend_on_their_state_alone(fp8_engine, fp8_diag, oracle):
    """The same bits at every row count (one tile, ragged tiles, both ring families, a full batch), under a permutation, under every
    bf16 kernel-choice switch (none of them may reach an fp8 result), after a second upload into the same model id, and between the
    shipped and the diagnostic library."""
    params = random_params(CH, seed=9)
    fp8_engine.net_set_params(4, params)
    fp8_diag.net_set_params(4, params)
    states = random_states(oracle, 8192, seed=77)
    ref_pi, ref_v = fp8_engine.predict_states(states, 4)
    try:
        for n in (1, 12, 13, 240, 241, 357, 1537, 3100, 8192):
            for t3, s3, nr, rp in ((1, 1, 32, 1), (0, 0, 0, 0), (1, 0, 8192, 0), (0, 1, 16, 1)):
                for key, val in (("conv3_tail", t3), ("conv3_small", s3), ("narrow_rows", nr), ("ring_packed", rp)):
                    fp8_engine.set_option(key, val)
                pi, v = fp8_engine.predict_states(states[:n], 4)
                assert np.array_equal(pi, ref_pi[:n]) and np.array_equal(v, ref_v[:n]), (n, t3, s3, nr, rp)
            perm = np.random.default_rng(n).permutation(n)
            pi, v = fp8_engine.predict_states(states[:n][perm], 4)
            assert np.array_equal(pi, ref_pi[:n][perm]) and np.array_equal(v, ref_v[:n][perm]), n
            pi, v = fp8_diag.predict_states(states[:n], 4)
            assert np.array_equal(pi, ref_pi[:n]) and np.array_equal(v, ref_v[:n]), n
    finally:
        for key, val in (("conv3_tail", 1), ("conv3_small", 1), ("narrow_rows", 32), ("ring_packed", 1)):
            fp8_engine.set_option(key, val)
    fp8_engine.net_set_params(4, random_params(CH, seed=10))             # other weights in between: the copies and scales follow
    other = fp8_engine.predict_states(states[:300], 4)
    assert not np.array_equal(other[0], ref_pi[:300])
    fp8_engine.net_set_params(4, params)
    pi, v = fp8_engine.predict_states(states[:300], 4)
    assert np.array_equal(pi, ref_pi[:300]) and np.array_equal(v, ref_v[:300])


def test_fp8_replay_parity_selfplay_with_refill(fp8_engine, oracle):
    """2048 episodes on 1024 slots at 100 simulations, fp8 on, tables + de-duplication + the evaluation cache on: every episode replays
    on the oracle from its own recorded rows, the recorded rows are what predict_states returns, and eval_dedup 0 plays the same games."""
    fp8_engine.net_init_random(24, seed=8)
    n, conc, sims, seed = 2048, 1024, 100, 44
    cap = 42 * (sims + 1) + 8
    fp8_engine.reset_stats()
    got = fp8_engine.selfplay(n_games=n, concurrent=conc, num_sims=sims, model_id=24, seed=seed, want_boards=False, record_evals=cap)
    st = fp8_engine.stats()
    assert st["games"] == n and st["leaf_rows_executed"] < st["leaf_rows_requested"]
    logs = fp8_engine.selfplay_get_evals(n, cap)
    assert logs[0].max() <= cap and logs[0].min() > 0
    _replay_every_episode(oracle, got, logs, sims, seed, n)
    cnt, states, pis, vs = logs                      # every row of 256 games spread over the ids (with 0, 17 and the last)
    assert_every_recorded_row_is_the_net(fp8_engine, 24, cnt, states, pis, vs, games=sorted(set(np.linspace(0, n - 1, 256).astype(int).tolist()) | {17}))
    try:
        fp8_engine.set_option("eval_dedup", 0)
        plain = fp8_engine.selfplay(n_games=n, concurrent=conc, num_sims=sims, model_id=24, seed=seed, want_boards=False)
    finally:
        fp8_engine.set_option("eval_dedup", 1)
    for key in ("moves", "game_len", "pis", "zs"):
        assert np.array_equal(plain[key], got[key]), key


def test_switching_the_class(engine_mod, oracle):
    """One model, a persistent evaluation cache, bf16 -> fp8 -> bf16: the first and third runs are identical tuple for tuple (no row of
    the other class is ever served), the second differs; the refusals; and two engines with different classes do not see each other."""
    a = engine_mod.Engine(device=0, max_batch=512, net_channels=128)
    b = engine_mod.Engine(device=0, max_batch=512, net_channels=128)
    try:
        for e in (a, b):
            e.net_init_random(0, seed=5)
        a.set_option("eval_cache_log2", 20)
        a.set_option("eval_cache_persist", 1)
        runs = []
        for fp8 in (0, 1, 0):
            a.set_option("net_fp8", fp8)
            runs.append(a.selfplay(n_games=64, num_sims=50, model_id=0, seed=3))
        for key in ("moves", "game_len", "pis", "zs", "boards"):
            assert np.array_equal(runs[0][key], runs[2][key]), key
        assert not (runs[0]["pis"].shape == runs[1]["pis"].shape and np.array_equal(runs[0]["pis"], runs[1]["pis"]))
        # refusals
        def refused(e, key, val):
            with pytest.raises(engine_mod.AzError) as ei:
                e.set_option(key, val)
            assert ei.value.status == AZ_ERR_BAD_ARGUMENT, (key, val)
            assert "net_fp8" in str(ei.value) or "conv2_table" in str(ei.value)
        a.set_option("net_fp8", 1)
        refused(a, "conv2_table", 0)
        a.set_option("net_fp8", 0)
        a.set_option("conv2_table", 0)
        refused(a, "net_fp8", 1)
        a.set_option("conv2_table", 1)
        a.selfplay_begin(n_games=8, concurrent=4, num_sims=25, model_id=0, seed=1)
        try:
            refused(a, "net_fp8", 1)
        finally:
            a.selfplay_end()
        # per engine
        st = random_states(oracle, 300, seed=9)
        ref_b = b.predict_states(st, 0)
        a.set_option("net_fp8", 1)
        ref_a = a.predict_states(st, 0)
        assert not np.array_equal(ref_a[0], ref_b[0])
        for k in range(3):
            ga, gb = a.predict_states(st, 0), b.predict_states(st, 0)
            assert np.array_equal(ga[0], ref_a[0]) and np.array_equal(ga[1], ref_a[1]), k
            assert np.array_equal(gb[0], ref_b[0]) and np.array_equal(gb[1], ref_b[1]), k
        b.set_option("net_fp8", 1)                       # the scales are a function of the weights alone: the same class, the same bits
        gb = b.predict_states(st, 0)
        assert np.array_equal(gb[0], ref_a[0]) and np.array_equal(gb[1], ref_a[1])
    finally:
        a.close()
        b.close()


def test_fp8_replay_parity_arena_with_two_conv_nets(fp8_engine, oracle):
    """az_arena with two conv nets, fp8 on (the old model's searches on the second stream and workspace, the shared tagged cache, small
    batches): 256 games at 100 simulations held to the oracle by replay parity."""
    fp8_engine.net_init_random(22, seed=5)
    fp8_engine.net_init_random(23, seed=6)
    num, sims = 256, 100
    cap = 22 * (sims + 1) + 8
    wld, res = fp8_engine.arena(num, sims, new_model_id=23, old_model_id=22, seed=9, record_evals=cap)
    assert int(wld.sum()) == num
    logs = [fp8_engine.arena_get_evals(w, num, cap) for w in (0, 1)]
    assert max(int(l[0].max()) for l in logs) <= cap
    sel = list(range(num))
    rn, ro = (_flatten_log(*logs[w], sel) for w in (0, 1))
    owld, ores, bad = oracle.arena_ex(num, sims, first_game=0, n_games=num, net_kind=oracle.NET_REPLAY, seed=9, threads=16, replay_new=rn, replay_old=ro)
    assert not bad.any(), np.flatnonzero(bad)[:5]
    assert np.array_equal(ores, res) and owld.tolist() == wld.tolist()
    glen, gmoves = fp8_engine.arena_get_moves(num)
    _check_move_record(oracle, glen, gmoves, res)
    for w, mid in ((0, 23), (1, 22)):                # every row of every game, under the right model
        assert_every_recorded_row_is_the_net(fp8_engine, mid, *logs[w])


@pytest.mark.parametrize("threads", [1, 2])
@pytest.mark.parametrize("graph", [0, 8, 20])        # 20: the shipped value (no graph at 16 simulations); 8: two graph replays per move
@pytest.mark.parametrize("dedup", [0, 1])
def test_fp8_every_row_of_a_draining_selfplay_is_the_net(fp8_engine, dedup, graph, threads):
    fp8_engine.net_init_random(25, seed=23)
    hold_a_draining_selfplay(fp8_engine, 25, dedup, graph, threads)


def test_fp8_every_row_of_an_arena_and_a_tree_search_is_the_net(fp8_engine, oracle):
    fp8_engine.net_init_random(26, seed=24)
    fp8_engine.net_init_random(27, seed=25)
    hold_an_arena_and_a_tree_search(fp8_engine, oracle, 26, 27)
