"""CPU tests of the layer-by-layer reference (tests/net_layers_ref.py) and of the two bounds the GPU layer tests use
(tests/test_net_layers_gpu.py): the reference agrees with the project's older whole-net reference and with itself in its two forms
of conv1 / conv2; an honest f32 "device twin" (another K order, one bf16 rounding) stays inside every bound; every mutation a
kernel could plausibly suffer breaks the random-data bound or the exact-data equality -- so the GPU tests can fail; and the
conditions under which exact data demand bit-for-bit results hold for the parameters and inputs the GPU tests use.  No GPU.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import net_layers_ref as L
from net_ref import exact_params, forward_ref, random_params
from test_net_gpu import random_states

C = 128
N_TWIN = 24


def conv1_pattern(mine, theirs, y, x):
    """A scalar transcription of the engine's conv1_pattern (csrc/az_net.hip)."""
    idx, mul = 0, 1
    for ky in range(3):
        for kx in range(3):
            iy, ix = y + ky - 1, x + kx - 1
            if 0 <= iy < 6 and 0 <= ix < 7:
                bit = 1 << (ix * 7 + (5 - iy))
                idx += (1 if mine & bit else 2 if theirs & bit else 0) * mul
            mul *= 3
    return idx


@pytest.fixture(scope="module")
def states(oracle):
    return L.layer_states(random_states, oracle)


@pytest.fixture(scope="module")
def rnd():
    """random_params at C = 128 on 24 arbitrary boards, layer by layer in float64 (each layer from the bf16 rounding before it)."""
    params = random_params(C, seed=3)
    folded = L.fold_like_engine(params, C)
    st = L.arbitrary_states(N_TWIN, seed=7)
    return params, folded, st, L.forward_layers(st, folded)


@pytest.fixture(scope="module")
def exa():
    params = exact_params(C, L.EXACT_SEED, L.HEAD_SHIFT[C])
    folded = L.fold_like_engine(params, C)
    st = L.arbitrary_states(N_TWIN, seed=7)
    return params, folded, st, L.forward_layers(st, folded)


def test_arbitrary_states_and_features(oracle, states):
    """arbitrary_states: disjoint planes, only the 42 board bits, all three cell values everywhere, floating stones; boards_of is the
    oracle's to_features; patterns_of is conv1_pattern at all 42 positions of legal and arbitrary boards."""
    arb = L.arbitrary_states(300, seed=1)
    board_bits = sum(1 << (x * 7 + (5 - y)) for y in range(6) for x in range(7))
    assert not (arb[:, 0] & arb[:, 1]).any() and not ((arb[:, 0] | arb[:, 1]) & np.uint64(~board_bits & (2 ** 64 - 1))).any()
    cell = L.cells_of(arb)
    assert all((cell == k).any(axis=0).all() for k in (0, 1, 2))
    assert ((cell[:, :-1] != 0) & (cell[:, 1:] == 0)).any()                      # a stone over an empty cell
    n_arb, n_legal = (len(np.unique(L.patterns_of(s))) for s in (arb, random_states(oracle, 300, seed=1)))
    print("distinct conv1 patterns on 300 boards: arbitrary", n_arb, "random legal play", n_legal)
    assert n_arb > 5000 and n_arb > 3 * n_legal                                  # 12600 uniform draws of 19683 leave ~9300 distinct at most
    assert np.array_equal(L.boards_of(states), np.stack([oracle.c4_features(int(m), int(t)) for m, t in states]))
    pat = L.patterns_of(states)
    for i in (0, 3, 40, 74, 75, 76, 120, 149):
        m, t = int(states[i, 0]), int(states[i, 1])
        assert [[conv1_pattern(m, t, y, x) for x in range(7)] for y in range(6)] == pat[i].tolist(), i
    assert pat.min() >= 0 and pat.max() < L.PATTERNS


def test_fold_is_the_whole_net_reference(rnd, states):
    """The layered reference chained end to end equals net_ref.forward_ref(emulate_bf16=True) within that file's bars (|dpi| 2e-3,
    |dv| 6e-3: two honest implementations of the same contract differ by flipped bf16 roundings at most)."""
    params, folded, _, _ = rnd
    out = L.forward_layers(states, folded)
    pi, v, _ = L.heads_ref(out["fc2"][2], folded)
    rpi, rv = forward_ref(params, L.boards_of(states), C, emulate_bf16=True)
    print("layered vs forward_ref: |dpi|", np.abs(pi - rpi).max(), "|dv|", np.abs(v - rv).max())
    assert np.abs(pi - rpi).max() <= 2e-3 and np.abs(v - rv).max() <= 6e-3


def test_conv1_table_is_conv1(rnd, exa, states):
    """Row conv1_pattern(s, y, x) of conv1_table_ref is conv1 of the board at (y, x), computed by an independent float64 convolution
    of the feature planes: legal and arbitrary boards, all 42 positions, edges included."""
    for _, folded, _, _ in (rnd, exa):
        T, S = L.conv1_table_ref(folded)
        assert T.shape == (L.PATTERNS, C) and (S >= np.abs(T)).all()
        w, b = folded["conv1"]
        wt = torch.from_numpy(w.astype(np.float64).reshape(3, 3, 2, C)).permute(3, 2, 0, 1).contiguous()
        y = torch.relu(F.conv2d(torch.from_numpy(L.boards_of(states).astype(np.float64)), wt, torch.from_numpy(b.astype(np.float64)), padding=1))
        y = y.permute(0, 2, 3, 1).numpy()
        got = L.conv1_rows(states, T)
        assert np.abs(got - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
        y2, S2 = L.conv1_ref(states, folded)
        assert np.array_equal(y2, got) and np.array_equal(S2, L.conv1_rows(states, S))


def test_table_conv2_is_conv2(rnd):
    """conv2 as the gather of U = T x W2 equals conv2's GEMM form: with U unrounded up to float64 summation order, with U rounded to
    f16 within the table bound (nine f16 roundings)."""
    _, folded, st, out = rnd
    T = L.bf16_round64(L.conv1_table_ref(folded)[0])
    y, S = L.layer_ref("conv2", L.conv1_rows(st, T), folded)

    def U_of(q, rounded):
        U = L.u_ref(T[q], folded)[0]
        return L.f16_from_bits(L.f16_bits(U)) if rounded else U
    yt, St = L.table_conv2_ref(lambda q: U_of(q, False), st, folded)
    assert np.abs(yt - y).max() <= 1e-12 * S.max()
    assert (St <= S + 1e-12).all()           # the gather's S sums |u| over its <= 9 terms: |sum a w| <= sum |a||w|
    yr, Sr = L.table_conv2_ref(lambda q: U_of(q, True), st, folded)
    # every in-board tap adds one f16 rounding: sum over taps of 2^-11 |u| + 2^-25 <= 2^-11 S + 9 * 2^-25
    assert (np.abs(yr - y) <= 2.0 ** -11 * S + 9 * 2.0 ** -25).all()
    assert not np.array_equal(yr, y)


# ---- the device twin --------------------------------------------------------------------------------------------------
def im2col(name, a):
    """[M][K] with K = tap * C + ci, as the kernels see a layer's input."""
    a = np.asarray(a, np.float32)
    if name in ("fc1", "fc2"):
        return a.reshape(a.shape[0], -1)
    if name == "conv2":
        a = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))
    n, h, w, c = a.shape
    return np.concatenate([a[:, ky:ky + h - 2, kx:kx + w - 2].reshape(-1, c) for ky in range(3) for kx in range(3)], axis=1)


def twin_layer(name, a_in, folded, seed, A=None, W=None, drop=None):
    """An honest f32 kernel: the K range in 32-wide blocks in a shuffled order, each block's partial product added to an f32
    accumulator, then + bias, ReLU, one bf16 rounding -> float64 values of the stored bf16.  A / W replace the operands (mutations);
    drop = a K range left out."""
    w, b = folded[name]
    A = im2col(name, a_in) if A is None else A
    W = np.asarray(w, np.float32) if W is None else W
    acc = np.zeros((A.shape[0], W.shape[1]), np.float32)
    for blk in np.random.default_rng(seed).permutation(A.shape[1] // 32):
        k = slice(blk * 32, blk * 32 + 32)
        if drop is not None and drop[0] <= k.start < drop[1]:
            continue
        acc = (acc + (A[:, k] @ W[k]).astype(np.float32)).astype(np.float32)
    shp = np.shape(a_in)
    out_shape = (shp[0], W.shape[1]) if name in ("fc1", "fc2") else (shp[0],) + ((6, 7) if name == "conv2" else (shp[1] - 2, shp[2] - 2)) + (W.shape[1],)
    return L.bf16_round64(np.maximum(acc + b, np.float32(0))).reshape(out_shape)


def test_device_twin_satisfies_every_bound(rnd, exa):
    """The bounds are not too tight for an honest kernel: an f32 twin of every stage stays inside the random-data bound, element for
    element, and reproduces exact data bit for bit."""
    _, folded, st, out = rnd
    # t1: bias then the <= 18 weight rows in the kernel's order, f32
    w1, b1 = folded["conv1"]
    T, S = L.conv1_table_ref(folded)
    q = np.arange(L.PATTERNS)
    acc = np.tile(b1, (L.PATTERNS, 1))
    for t in range(9):
        d = (q // 3 ** t) % 3
        for ci in range(2):
            acc = (acc + (d == ci + 1)[:, None] * w1[t * 2 + ci]).astype(np.float32)
    t1 = L.bf16_round64(np.maximum(acc, 0))
    assert L.worst_ratio(t1, T, L.bound_bf16(T, S, 18)) <= 1
    # u2 from the twin's own t1, f16; then the gather over the twin's u2
    rows = np.unique(L.patterns_of(st))
    U, SU = L.u_ref(t1[rows], folded)
    w2 = folded["conv2"][0].reshape(9, C, C)
    u_dev = np.stack([(t1[rows].astype(np.float32)[:, ::-1] @ w2[t][::-1]) for t in range(9)], axis=1).astype(np.float16)
    assert L.worst_ratio(u_dev.astype(np.float64), U, L.bound_f16(U, SU, C)) <= 1
    lut = {int(p): i for i, p in enumerate(rows)}
    U_of = lambda qs: u_dev[[lut[int(p)] for p in qs]].astype(np.float64)
    y, S2 = L.table_conv2_ref(U_of, st, folded)
    a2 = L.bf16_round64(y.astype(np.float32))                     # (the sum of <= 9 f16 values and a bias: f32 order errors below the bound by far)
    assert L.worst_ratio(a2, y, L.bound_bf16(y, S2, 9)) <= 1
    # the GEMM layers, each from the reference's stored input
    a = out["t1"]
    for i, name in enumerate(L.LAYERS):
        y, S, stored = out[name]
        r = L.worst_ratio(twin_layer(name, a, folded, seed=i), y, L.bound_bf16(y, S, L.layer_k(name, C)))
        print("twin", name, "err / bound", r)
        assert r <= 1, name
        a = stored
    # heads in f32
    x = out["fc2"][2]
    pi, v, lb = L.heads_ref(x, folded)
    x32 = x.astype(np.float32)
    lp, lv = x32 @ folded["pi"][0] + folded["pi"][1], x32 @ folded["v"][0] + folded["v"][1]
    assert (np.abs(torch.softmax(torch.from_numpy(lp), 1).numpy() - pi) <= 0.5 * lb[:, None] + 1e-6).all()
    assert (np.abs(np.tanh(lv) - v) <= lb + 1e-6).all()
    # exact data: bit for bit, in any order
    _, efolded, _, eout = exa
    a = eout["t1"]
    for i, name in enumerate(L.LAYERS):
        assert np.array_equal(twin_layer(name, a, efolded, seed=10 + i), eout[name][2]), name
        a = eout[name][2]


def test_mutations_are_caught(rnd, exa):
    """conv3 at C = 128 on 24 arbitrary boards.  Each of these, applied to the twin, must exceed the random-data bound somewhere; the
    one the random-data bound cannot see -- a single dropped input channel of one tap -- must change exact data."""
    _, folded, _, out = rnd
    a_in, (y, S, _) = out["conv2"][2], out["conv3"]
    bound = L.bound_bf16(y, S, 9 * C)
    A, W = im2col("conv3", a_in), folded["conv3"][0]
    assert L.worst_ratio(twin_layer("conv3", a_in, folded, 1), y, bound) <= 1

    def swapped_taps():
        W2 = W.copy()
        W2[2 * C:3 * C], W2[5 * C:6 * C] = W[5 * C:6 * C], W[2 * C:3 * C]
        return twin_layer("conv3", a_in, folded, 1, W=W2)

    def neighbour_channel():
        a2 = np.array(a_in)
        a2[..., 17] = a_in[..., 18]
        return twin_layer("conv3", a2, folded, 1)

    def next_board():
        got = twin_layer("conv3", a_in, folded, 1)
        got[5] = got[6]
        return got

    def four_ulp():
        bits = L.bf16_bits(twin_layer("conv3", a_in, folded, 1)).copy()
        bits[..., int(y.reshape(-1, C).mean(axis=0).argmax())] += np.uint16(4)        # a live channel (a dead one stores zeros: +4 is a denormal)
        return L.bf16_from_bits(bits)

    def dropped_term(a, f):
        A2 = im2col("conv3", a).copy()
        A2[:, 4 * C + 9] = 0
        return twin_layer("conv3", a, f, 1, A=A2)

    mutations = {"dropped 64-channel K-step": lambda: twin_layer("conv3", a_in, folded, 1, drop=(3 * C + 64, 3 * C + 128)),
                 "two taps swapped": swapped_taps, "one input channel from its neighbour": neighbour_channel,
                 "one board's rows from the next board": next_board, "one output channel off by 4 bf16 ulp": four_ulp}
    for name, f in mutations.items():
        got = f()
        err = np.abs(got - y)
        print(f"{name}: {float((err > bound).mean()):.3f} of outputs over the bound, worst ratio {L.worst_ratio(got, y, bound):.1f}")
        assert (err > bound).any(), name
    got = dropped_term(a_in, folded)
    print("one dropped input channel of one tap, random data: worst ratio", L.worst_ratio(got, y, bound))
    # ... exact data see every one of them, the single dropped term included
    _, efolded, _, eout = exa
    ea, estored = eout["conv2"][2], eout["conv3"][2]
    assert np.array_equal(twin_layer("conv3", ea, efolded, 1), estored)
    got = dropped_term(ea, efolded)
    assert not np.array_equal(got, estored)
    print("one dropped input channel of one tap, exact data: outputs that differ", int((got != estored).sum()))
    assert not np.array_equal(twin_layer("conv3", ea, efolded, 1, drop=(3 * C + 64, 3 * C + 128)), estored)


@pytest.mark.parametrize("channels", [128, 256, 384, 512])
def test_exact_data_conditions(states, channels):
    """What makes "bit for bit" a fair demand, for the parameter seed and the inputs of the GPU tests: every layer's S < 2^24 (any f32
    order is exact), every conv2-table entry an integer of at most 2048 (exact in f16), every layer alive, heads unsaturated; and the
    f32 evaluation of the reference equals the float64 one."""
    params = exact_params(channels, L.EXACT_SEED, L.HEAD_SHIFT[channels])
    folded = L.fold_like_engine(params, channels)
    for name in ("conv1",) + L.LAYERS:                  # BatchNorm folds to exactly 1: the folded parameters are the integers
        w, b = folded[name]
        assert np.array_equal(w, np.rint(w)) and np.array_equal(b, np.rint(b)), name
    out = L.forward_layers(states, folded, dtype=torch.float32)
    pi, v, _ = L.heads_ref(out["fc2"][2], folded)
    L.exact_conditions(out, pi, v)
    out8 = L.forward_layers(states[:8], folded)
    for name in L.LAYERS:
        assert np.array_equal(out8[name][0], out[name][0][:8]) and np.array_equal(out8[name][1], out[name][1][:8]), name
    T, S = L.conv1_table_ref(folded)
    assert S.max() < 2 ** 24 and np.array_equal(T, L.bf16_round64(T))
    rows = L.u2_rows(channels)[:-1]
    U, SU = L.u_ref(T[rows], folded, dtype=torch.float32)
    assert SU.max() <= 2048 and np.array_equal(U, np.rint(U))
    tab = L.table_conv2_ref(lambda q: L.u_ref(T[q], folded, dtype=torch.float32)[0], states, folded)
    assert np.array_equal(tab[0], out["conv2"][0])           # on exact data the table and the GEMM form of conv2 are the same numbers
    print(channels, "max S per layer", out["S1"], [float(out[n][1].max()) for n in L.LAYERS], "largest |u2|", np.abs(U).max(),
          "pi", pi.min(), pi.max(), "|v|", np.abs(v).max())
