"""GPU tests that hold EVERY LAYER of the default bf16 inference net, and both per-model conv tables, to the float64 layer-by-layer
reference of tests/net_layers_ref.py -- element for element, with bounds that are derived, not measured (that module's docstring;
tests/test_net_layers_cpu.py shows that an honest f32 kernel meets them and that a dropped K-step, swapped taps, a wrong channel, a
wrong board's rows or a 4-ulp offset do not).  tests/test_net_gpu.py compares (pi, v) only, six layers later.

How a layer is read: the diagnostic library's az_diag_read_act / az_diag_read_conv_table copy stream 0's workspace and a model's
tables.  az_net_predict_states with B <= max_batch runs ONE forward with the rows in the caller's order -- no de-duplication, and
"eval_mirror" is off -- so workspace row i is state i.

  exact data   integer parameters (net_ref.exact_params): act2 .. fc2o, t1 and u2 must be the reference's bits, at every width
               that takes other kernel templates, every row count around the kernels' hand-overs, under every kernel-set option.
  random data  random_params, teacher-forced: layer l's reference is computed from what the reader returned for layer l - 1, so
               each comparison isolates one kernel; |dev - y| <= 2^-8 |y| + (K + 1) 2^-23 S for every element.

Largest err / bound seen on the MI355X (information, not the bar -- the bar is 1; t1 and the table gather sit at bf16's half ulp):
  C = 128, conv2_table 1: t1 0.995  u2 0.937  conv2 0.995  conv3 0.820  conv4 0.818  fc1 0.887  fc2 0.813  pi, v < 5e-4 (all four runs)
  C = 128, conv2_table 0: conv2 0.880  conv3 0.812  conv4 0.817  fc1 0.890  fc2 0.834
  C = 512, conv2_table 1: t1 0.995  u2 0.721  conv2 0.996  conv3 0.426  conv4 0.371  fc1 0.549  fc2 0.793
  C = 512, conv2_table 0: conv2 0.551  conv3 0.429  conv4 0.370  fc1 0.523  fc2 0.789
  tables, all rows: u2 0.947 / 0.888 / 0.734 at C = 128 / 256 / 512; conv1 x 2^k, k = -12 .. 12: the same figures for every k.
Exact data: no bit differed, at any width, row count or option set.

The row counts here stop at 150 with max_batch = 256, and predict_states can only run a forward whose bound is its exact count and
which has no estimate.  Above that -- the image-resident conv3 kernel past one round and its cut tail, the ring's two-per-CU family
and its 96 .. 192-row tiles, the FCs' family window -- and for every (exact count, bound, estimate) a search can hand the launchers,
tests/test_net_routes_gpu.py holds the same layers to the same exact reference on a pool of 8192 states (the triples: tests/net_routes.py).
"""
import ctypes

import numpy as np
import pytest
import torch

import net_layers_ref as L
from net_ref import exact_params, layout, random_params
from test_net_gpu import random_states

pytestmark = pytest.mark.gpu

ROWS = (1, 13, 33, 65, 129, 150)     # 13: one full + one ragged 12-board image tile; 33 / 65 / 129: one past the skinny hand-over of
                                     # conv3 / conv4 / the FCs and one past a 128-row ring tile
DEFAULTS = {"conv2_table": 1, "conv1_table": 1, "conv3_small": 1, "narrow_rows": 32, "conv3_wreg": 1, "conv3_planes": 1, "conv3_tail": 1,
            "ring_packed": 1, "gemm_variant": 5, "fc_ring": 1, "conv3_ring": 0}
OPTION_SETS = ([{}, {"conv2_table": 0, "conv1_table": 0}]
               + [{"conv3_small": 0, "narrow_rows": 0, "conv3_wreg": w, "conv3_planes": p, "conv3_tail": t} for w in (0, 1) for p in (0, 1) for t in (0, 1)]
               + [{"narrow_rows": 8192}, {"ring_packed": 0}, {"gemm_variant": 0}, {"fc_ring": 0}, {"conv3_ring": 1}])
ACT_SHAPE = {1: lambda c: (8, 9, c), 2: lambda c: (6, 7, c), 3: lambda c: (4, 5, c), 4: lambda c: (2, 3, c), 5: lambda c: (1024,), 6: lambda c: (512,)}
LAYER_NO = {"conv2": 2, "conv3": 3, "conv4": 4, "fc1": 5, "fc2": 6}


def read_act(e, layer, rows, channels):
    """Layer `layer`'s activations of the engine's last forward as uint16 bf16 bits, [rows] + the layer's shape; None where the
    reader refuses (-1)."""
    f = e._lib.az_diag_read_act
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    out = np.empty((rows,) + ACT_SHAPE[layer](channels), np.uint16)
    got = f(e._h, layer, rows, out.ctypes.data_as(ctypes.c_void_p))
    if got == -1:
        return None
    assert got == out.nbytes, (got, out.nbytes)
    return out


def refused_act(e, layer, rows):
    """az_diag_read_act answers -1 (nothing is copied: a small buffer will do)."""
    f = e._lib.az_diag_read_act
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return f(e._h, layer, rows, np.empty(16, np.uint16).ctypes.data_as(ctypes.c_void_p)) == -1


def read_table(e, model_id, which, first, n, channels):
    """Rows [first, first + n) of a model's t1 (which = 1: [n][C] bf16 bits) or u2 (2: [n][9][C] f16 bits); None where refused."""
    f = e._lib.az_diag_read_conv_table
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    out = np.empty((max(n, 2), 9 if which == 2 else 1, channels), np.uint16)[:max(n, 0)]      # (room for what a refused call asks for)
    out = out.reshape((-1, channels) if which != 2 else (-1, 9, channels))
    got = f(e._h, model_id, which, first, n, out.ctypes.data_as(ctypes.c_void_p))
    if got == -1:
        return None
    assert n > 0 and got == out.nbytes, (got, out.nbytes)
    return out


def read_u2_rows(e, model_id, rows, channels):
    """The u2 rows `rows` (sorted, distinct), consecutive runs in one copy each."""
    rows = np.asarray(rows)
    out = np.empty((len(rows), 9, channels), np.uint16)
    cuts = np.flatnonzero(np.diff(rows) != 1) + 1
    o = 0
    for run in np.split(rows, cuts):
        out[o:o + len(run)] = read_table(e, model_id, 2, int(run[0]), len(run), channels)
        o += len(run)
    return out


def set_options(e, opts):
    for k, v in {**DEFAULTS, **opts}.items():
        e.set_option(k, v)


@pytest.fixture(scope="module")
def states(oracle):
    st = L.layer_states(random_states, oracle)
    assert st.shape == (150, 2) and not (st[:, 0] & st[:, 1]).any()
    return st


# ---- exact data ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [128, 256, 384, 512])
def test_exact_data_every_layer_bit_for_bit(engine_mod, states, channels):
    """Widths 128 / 256 / 384 / 512 take different templates (k_gemm_mfma<1> vs the image-resident conv2 GEMM, skinny depth 8 / 6 / 2,
    1 - 4 conv3 column tiles).  The reference is computed once; its conditions (S < 2^24 per layer, alive layers, unsaturated heads)
    are asserted from the reference alone before the device is looked at.  On exact data u2 is exact, so conv2 as a table and as a
    GEMM must give the SAME act2 bits (on random data they round differently)."""
    params = exact_params(channels, L.EXACT_SEED, L.HEAD_SHIFT[channels])
    folded = L.fold_like_engine(params, channels)
    ref = L.forward_layers(states, folded, dtype=torch.float32)
    rpi, rv, _ = L.heads_ref(ref["fc2"][2], folded)
    L.exact_conditions(ref, rpi, rv)
    ref8 = L.forward_layers(states[:8], folded)                      # the f32 evaluation is the float64 one
    assert all(np.array_equal(ref8[k][0], ref[k][0][:8]) and np.array_equal(ref8[k][1], ref[k][1][:8]) for k in L.LAYERS)
    want = {LAYER_NO[k]: L.bf16_bits(ref[k][2]) for k in L.LAYERS}
    want_t1 = L.bf16_bits(ref["t1"])
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=channels, diag=True)
    shipped = engine_mod.Engine(device=0, max_batch=256, net_channels=channels)
    try:
        e.net_set_params(0, params)
        shipped.net_set_params(0, params)
        pi0, v0 = e.predict_states(states, 0)
        assert read_act(e, 1, 1, channels) is None                     # act1 is not allocated until a kernel set needs it
        for layer, rows in ((0, 1), (7, 1), (2, 0), (2, -1), (2, 257)):   # the reader's bounds: no such layer, no rows, more than max_batch
            assert refused_act(e, layer, rows), (layer, rows)
        try:
            for opts in OPTION_SETS:
                set_options(e, opts)
                for n in ROWS:
                    pi, v = e.predict_states(states[:n], 0)
                    for layer, bits in want.items():
                        got = read_act(e, layer, n, channels)
                        if not np.array_equal(got, bits[:n]):
                            bad = np.argwhere(got != bits[:n])
                            raise AssertionError((channels, opts, n, "layer", layer, "elements that differ", len(bad), "first", bad[:4].tolist(),
                                                  "boards", np.unique(bad[:, 0])[:8].tolist(), "channels", np.unique(bad[:, -1])[:8].tolist()))
                    # the heads on the device's own fc2o (== the reference's): what is left is exp / tanh
                    assert np.abs(pi - rpi[:n]).max() <= 1e-6 and np.abs(v - rv[:n]).max() <= 1e-6, (opts, n)
                    assert np.array_equal(pi, pi0[:n]) and np.array_equal(v, v0[:n]), (opts, n)
                    if opts.get("conv1_table") == 0:                  # k_conv1 wrote act1: interior == t1[pattern], the halo zero
                        a1 = read_act(e, 1, n, channels)
                        assert np.array_equal(a1[:, 1:7, 1:8], want_t1[:n]), (opts, n)
                        halo = a1.copy()
                        halo[:, 1:7, 1:8] = 0
                        assert not halo.any(), (opts, n)
        finally:
            set_options(e, {})
        # the shipped library on the same states: the same bits, and NNet::predict on the planes is predict_states
        spi, sv = shipped.predict_states(states, 0)
        assert np.abs(spi - rpi).max() <= 1e-6 and np.abs(sv - rv).max() <= 1e-6
        assert np.array_equal(spi, pi0) and np.array_equal(sv, v0)
        ppi, pv = shipped.predict(L.boards_of(states), 0)
        assert np.array_equal(ppi, spi) and np.array_equal(pv, sv)
    finally:
        e.close()
        shipped.close()


# ---- the tables ---------------------------------------------------------------------------------------------------------
def check_tables(e, model_id, params, channels, exact, tag):
    """t1: all 19683 rows.  u2: net_layers_ref.u2_rows (all 19684 up to C = 256).  exact: bit for bit; else within the bounds, u2 from
    the device's own t1.  Returns (t1 bits, u2 bits)."""
    folded = L.fold_like_engine(params, channels)
    T, S = L.conv1_table_ref(folded)
    t1 = read_table(e, model_id, 1, 0, L.PATTERNS, channels)
    rows = L.u2_rows(channels)
    assert rows[-1] == L.PATTERNS and (rows[:-1] < L.PATTERNS).all()
    u2 = read_u2_rows(e, model_id, rows, channels)
    assert not u2[-1].any(), tag                                        # the appended zero row
    rows, u2v = rows[:-1], L.f16_from_bits(u2[:-1])
    if exact:
        assert S.max() < 2 ** 24
        assert np.array_equal(t1, L.bf16_bits(T)), (tag, "t1 rows that differ", np.unique(np.argwhere(t1 != L.bf16_bits(T))[:, 0])[:8])
        U, SU = L.u_ref(L.bf16_round64(T)[rows], folded, dtype=torch.float32)
        assert SU.max() <= 2048 and np.array_equal(U, np.rint(U))       # integers of at most 2048: exact in f16 in any f32 order
        want = L.f16_bits(U)
        want[want == 0x8000] = 0                                        # (a sum of integers is never -0)
        assert np.array_equal(u2[:-1], want), (tag, "u2 rows that differ", rows[np.unique(np.argwhere(u2[:-1] != want)[:, 0])][:8])
    else:
        r1 = L.worst_ratio(L.bf16_from_bits(t1), T, L.bound_bf16(T, S, 18))
        U, SU = L.u_ref(L.bf16_from_bits(t1)[rows], folded)
        assert np.abs(U).max() + L.bound_f16(U, SU, channels).max() < 65504     # finite in f16, says the reference
        r2 = L.worst_ratio(u2v, U, L.bound_f16(U, SU, channels))
        print(f"tables C={channels} {tag}: err / bound t1 {r1:.3f} u2 {r2:.3f}")
        assert r1 <= 1 and r2 <= 1, (tag, r1, r2)
    return t1, u2


@pytest.mark.parametrize("channels", [128, 256, 512])
def test_conv_tables_every_row(engine_mod, channels):
    """Both tables are rebuilt at every weight upload (k_conv1_table, then k_gemm_mfma<6> over 19683 = 153 * 128 + 99 rows) and play
    only ever reads ~4000 of the patterns.  Here: every t1 row, every u2 row (a subset at C = 512 that keeps the last two GEMM
    tiles), exact parameters bit for bit, random parameters within the bounds -- each upload into the SAME model id, so the tables
    must follow the weights."""
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=channels, diag=True)
    try:
        assert read_table(e, 3, 1, 0, 1, channels) is None              # no such model
        e.net_init_random(3, seed=1)
        for which, first, n in ((0, 0, 1), (3, 0, 1), (1, -1, 1), (1, 0, 0), (1, L.PATTERNS, 1), (1, L.PATTERNS - 1, 2), (2, L.PATTERNS + 1, 1), (2, L.PATTERNS, 2)):
            assert read_table(e, 3, which, first, n, channels) is None, (which, first, n)      # the reader's bounds
        check_tables(e, 3, _upload(e, 3, exact_params(channels, L.EXACT_SEED, L.HEAD_SHIFT[channels])), channels, True, "exact")
        a = check_tables(e, 3, _upload(e, 3, random_params(channels, seed=31)), channels, False, "second upload")
        b = check_tables(e, 3, _upload(e, 3, random_params(channels, seed=32)), channels, False, "third upload")
        assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    finally:
        e.close()


def _upload(e, model_id, params):
    e.net_set_params(model_id, params)
    return params


# ---- random data, teacher-forced ----------------------------------------------------------------------------------------
def check_teacher_forced(e, model_id, params, states, channels, table, tag):
    """One forward of `states`; every layer and the heads within the random-data bound of the reference computed from the DEVICE's
    own input to that layer, every element.  Returns {stage: largest err / bound}."""
    n = len(states)
    folded = L.fold_like_engine(params, channels)
    pi, v = e.predict_states(states, model_id)
    assert np.isfinite(pi).all() and np.isfinite(v).all(), tag
    acts = {layer: L.bf16_from_bits(read_act(e, layer, n, channels)) for layer in range(2, 7)}
    ratios = {}
    # conv1: the table rows (k_conv1's rows are the table's bits), K = 18
    T, S1 = L.conv1_table_ref(folded)
    t1 = L.bf16_from_bits(read_table(e, model_id, 1, 0, L.PATTERNS, channels))
    ratios["t1"] = L.worst_ratio(t1, T, L.bound_bf16(T, S1, 18))
    a1 = read_act(e, 1, n, channels) if not table else None
    if a1 is not None and channels % 256 != 0:                         # conv2 as a GEMM read k_conv1's act1 (C % 256: the table rows)
        assert np.array_equal(L.bf16_from_bits(a1[:, 1:7, 1:8]), L.conv1_rows(states, t1)), tag
    if table:                                                          # u2 from the device's t1, then the gather over the device's u2
        pats = np.unique(L.patterns_of(states))
        u2 = L.f16_from_bits(read_u2_rows(e, model_id, pats, channels))
        U, SU = L.u_ref(t1[pats], folded)
        assert np.abs(U).max() + L.bound_f16(U, SU, channels).max() < 65504, tag
        ratios["u2"] = L.worst_ratio(u2, U, L.bound_f16(U, SU, channels))
        lut = np.full(L.PATTERNS, -1)
        lut[pats] = np.arange(len(pats))
        y, S = L.table_conv2_ref(lambda q: u2[lut[q]], states, folded)
        ratios["conv2"] = L.worst_ratio(acts[2], y, L.bound_bf16(y, S, 9))
    else:
        y, S = L.layer_ref("conv2", L.conv1_rows(states, t1), folded)
        ratios["conv2"] = L.worst_ratio(acts[2], y, L.bound_bf16(y, S, 9 * channels))
    for name in L.LAYERS[1:]:
        layer = LAYER_NO[name]
        y, S = L.layer_ref(name, acts[layer - 1], folded)
        ratios[name] = L.worst_ratio(acts[layer].reshape(y.shape), y, L.bound_bf16(y, S, L.layer_k(name, channels)))
    rpi, rv, lb = L.heads_ref(acts[6], folded)
    ratios["pi"] = float((np.abs(pi - rpi) / (0.5 * lb[:, None] + 1e-6)).max())
    ratios["v"] = float((np.abs(v - rv) / (lb + 1e-6)).max())
    print(f"teacher-forced C={channels} {tag}: err / bound " + " ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1, (tag, k, r)
    return ratios


@pytest.mark.parametrize("channels", [128, 512])
def test_random_data_every_layer_teacher_forced(engine_mod, states, channels):
    params = random_params(channels, seed=40 + channels)
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=channels, diag=True)
    try:
        e.net_set_params(1, params)
        try:
            for table in (1, 0):
                set_options(e, {"conv2_table": table})
                check_teacher_forced(e, 1, params, states, channels, table, f"conv2_table {table}")
        finally:
            set_options(e, {})
    finally:
        e.close()


@pytest.mark.parametrize("k", [-12, -6, 6, 12])
def test_scale_of_conv1_activations(engine_mod, states, k):
    """The same function with other numbers: conv1's BatchNorm gamma and beta times 2^k, conv2's weights over 2^k.  t1 moves by 2^k,
    W2 by 2^-k, and u2 = W2 x t1 -- the f16 numbers the table set lives on -- does not move at all: the table set's range is a
    range of conv2's per-tap partial sums (|u| < 65504; relative 2^-11 only above f16's normal threshold 2^-14, absolute 2^-25
    below), not of conv1's activations.  Wherever the reference says u2 is finite the bounds must hold and (pi, v) be finite."""
    channels = 128
    params = random_params(channels, seed=50)
    off, _ = layout(channels)
    o, _ = off["conv1_bn"]
    params[o:o + 2 * channels] *= np.float32(2.0 ** k)
    o, shp = off["conv2_w"]
    params[o:o + int(np.prod(shp))] *= np.float32(2.0 ** -k)
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=channels, diag=True)
    try:
        e.net_set_params(1, params)
        check_teacher_forced(e, 1, params, states, channels, 1, f"conv1 x 2^{k}")
    finally:
        e.close()
