"""CPU tests of the fp8 layer-by-layer reference (tests/net_layers_ref_fp8.py) and of the bounds the GPU layer tests of the "net_fp8"
class use (tests/test_net_layers_fp8_gpu.py): honest f32 kernels -- three summation orders -- stay inside every element's interval
and land on the nearest code; every mutation a kernel could plausibly suffer leaves it somewhere, so the GPU tests can fail; the
intervals are not vacuous (the share of elements with more than one accepted code is capped, from the reference alone); and the
conditions under which exact data demand bit-for-bit results hold at all four widths.  No GPU.

The widths, parameters and inputs are the GPU test's (random_params(C, 40 + C) on net_layers_ref.layer_states), cut to a few boards
where a few are enough; the activation scales are calibrated on the same inputs by the engine's rule (the GPU test passes the
engine's own).
"""
import numpy as np
import pytest
import torch

import net_layers_ref as L
import net_layers_ref_fp8 as L8
import net_ref_fp8 as r8
from net_ref import exact_params, random_params, unpack
from test_net_gpu import random_states

N_HONEST = 8          # boards of the honest-order test: 81920 conv3 outputs at C = 512
N_MUTANT = 6          # boards of the mutants: 120 conv3 rows = 7 full 16-row tiles and a ragged one of 8; 36 conv4 rows = 2 and 4


@pytest.fixture(scope="module")
def states(oracle):
    return L.layer_states(random_states, oracle)


_RND = {}


def rnd(states, C):
    """random_params(C, 40 + C) on all 150 states, computed once: conv2's codes by the exact gather over the reference's own f16 table
    rows, then conv3 and conv4 each from the stored codes of the layer before."""
    if C not in _RND:
        params = random_params(C, seed=40 + C)
        sa2, sa3 = r8.calibrate_scales(params, L.boards_of(states), C)
        folded = L.fold_like_engine(params, C)
        q = L8.quantised(params, C, sa2, sa3)
        T = L.bf16_round64(L.conv1_table_ref(folded)[0])
        pats = np.unique(L.patterns_of(states))
        U = L.f16_bits(L.u_ref(T[pats], folded)[0])
        lut = np.full(L.PATTERNS, -1)
        lut[pats] = np.arange(len(pats))
        U_of = lambda p: U[lut[p]]
        codes2, max2 = L8.conv2_codes_ref(U_of, states, folded, sa2)
        y3, beta3, _ = L8.layer8_ref("conv3", L8.code_values(codes2), q)
        codes3 = L8.nearest_codes(y3, sa3)
        y4, beta4, _ = L8.layer8_ref("conv4", L8.code_values(codes3), q)
        _RND[C] = dict(params=params, sa2=sa2, sa3=sa3, folded=folded, q=q, U_of=U_of, T=T, codes2=codes2, max2=max2, y3=y3, beta3=beta3,
                       codes3=codes3, y4=y4, beta4=beta4)
    return _RND[C]


@pytest.mark.parametrize("C", [128, 512])
def test_the_intervals_are_not_vacuous(states, C):
    """From the reference alone, on the GPU test's inputs: the share of conv3 elements with more than one accepted code stays under
    the cap (0.10 at C = 128, 0.35 at 512), the layers are alive, nothing saturates, and the reference's conv2 agrees with the
    emulation of net_ref_fp8 (two implementations of the same contract: at most a rare code one step away)."""
    r = rnd(states, C)
    share, share2, alive = L8.nonvacuous(r["y3"], r["beta3"], r["sa3"], L8.SHARE_CAP[C])
    print(f"C {C}: scales {r['sa2']} {r['sa3']}; conv3 elements with > 1 accepted code {share:.4f}, > 2 {share2:.4f}, nonzero {alive:.3f}; "
          f"largest scaled conv2 {r['max2']:.1f}, conv3 {float((np.maximum(r['y3'] + r['beta3'], 0) * r['sa3']).max()):.1f} of 448")
    assert r["max2"] < L8.FP8_MAX and (r["codes2"] != 0).mean() > 0.1 and np.unique(r["codes2"]).size > 16
    assert (r["y4"] > 0).mean() > 0.1
    rel = L8.conv4_bound(r["y4"], r["beta4"])[r["y4"] > 0] / r["y4"][r["y4"] > 0]
    print(f"C {C}: conv4 bound / value, median {np.median(rel):.2e}")
    assert np.median(rel) < 2.0 ** -5                      # the conv4 bound is a few bf16 ulps of the value, not a multiple of it
    P = unpack(np.asarray(r["params"], np.float32), C)
    with torch.no_grad():
        emu2 = r8.e4m3_codes(r8._front(P, torch.from_numpy(L.boards_of(states[:24]))) * np.float32(r["sa2"])).permute(0, 2, 3, 1).numpy()
    d = emu2.astype(int) - r["codes2"][:24]
    print(f"C {C}: conv2 codes that differ from the emulation's {int((d != 0).sum())} of {d.size}")
    assert (np.abs(d) <= 1).all() and (d != 0).mean() < 1e-3


def honest(name, a_codes, r, order, C):
    """An honest f32 kernel of conv3 / conv4 on e4m3 input codes -> the epilogue's f32 output [n][oh][ow][C]."""
    qw, dq, b, _ = r["q"][name]
    a = L8.code_values(a_codes)
    if order == "torch":
        acc = L8.acc_torch_f32(a, qw)
    else:
        acc = (L8.acc_sequential_f32 if order == "sequential" else L8.acc_blocks_f32)(L8.im2col(name, a), qw, C)
    return L8.epilogue_f32(acc, dq, b).reshape(a.shape[0], a.shape[1] - 2, a.shape[2] - 2, C)


@pytest.mark.parametrize("C", [128, 512])
def test_honest_f32_kernels_are_inside_every_interval(states, C):
    """conv3 and conv4 in f32 in three orders -- strictly sequential in the engine's K order (channel block outer, tap inner), exact
    128-product blocks accumulated in f32 (the MFMA's shape), torch's own f32 convolution -- from the reference's stored inputs:
    every element inside its interval.  Printed: how many conv3 codes are not the nearest one (the yardstick the GPU test compares
    the device's counts with; measured: none, in the first two orders, at both widths)."""
    r = rnd(states, C)
    n = N_HONEST
    lo, hi = L8.accepted_codes(r["y3"][:n], r["beta3"][:n], r["sa3"])
    near = L8.nearest_codes(r["y3"][:n], r["sa3"])
    for order in ("sequential", "blocks", "torch"):
        got = L8.store_conv3(honest("conv3", r["codes2"][:n], r, order, C), r["sa3"])
        off, one = L8.off_nearest(got, near)
        print(f"C {C} conv3 {order}: codes off the nearest one {off} of {got.size} ({one} of them one step away)")
        assert L8.inside(got, lo, hi).all(), order
        if order != "torch":
            assert off == 0, (order, off)
        r4 = honest("conv4", r["codes3"][:n], r, order, C)
        ratio = L.worst_ratio(L.bf16_round64(r4), np.maximum(r["y4"][:n], 0.0), L8.conv4_bound(r["y4"][:n], r["beta4"][:n]))
        print(f"C {C} conv4 {order}: err / bound {ratio:.3f}")
        assert ratio <= 1, order


def conv3_mutants(r, C, n):
    """name -> codes [n][4][5][C] of a wrong conv3 kernel (the honest block-order kernel with one thing changed)."""
    qw, dq, b, _ = r["q"]["conv3"]
    A = L8.im2col("conv3", L8.code_values(r["codes2"][:n]))
    shape = (n, 4, 5, C)
    fin = lambda acc, dq_=dq, b_=b, sa=r["sa3"]: L8.store_conv3(L8.epilogue_f32(acc, dq_, b_), sa).reshape(shape)
    good_acc = L8.acc_blocks_f32(A, qw, C)
    good = fin(good_acc)
    out = {}
    out["one dropped K-step (tap 4, channels 0..127)"] = fin(L8.acc_blocks_f32(A, qw, C, skip=(4, 0)))
    W2 = qw.copy()
    W2[2 * C:3 * C], W2[5 * C:6 * C] = qw[5 * C:6 * C], qw[2 * C:3 * C]
    out["two taps swapped"] = fin(L8.acc_blocks_f32(A, W2, C))
    A2 = A.copy().reshape(A.shape[0], -1, 8, 16)              # [M][K-step][16-byte chunk][byte]
    A2[:, :, [1, 5]] = A2[:, :, [5, 1]]
    out["16-byte chunks 1 and 5 swapped in the activations only"] = fin(L8.acc_blocks_f32(A2.reshape(A.shape), qw, C))
    assert (dq != np.roll(dq, -1)).any() and (b != np.roll(b, -1)).any()
    out["channel n with channel n + 1's dq"] = fin(good_acc, dq_=np.roll(dq, -1))
    out["channel n with channel n + 1's bias"] = fin(good_acc, b_=np.roll(b, -1))
    if r["sa2"] != r["sa3"]:
        out["sa2 used for sa3"] = fin(good_acc, sa=r["sa2"])
    out["truncation in place of round-to-nearest-even"] = L8.codes_truncated(
        L8.epilogue_f32(good_acc, dq, b).astype(np.float64) * r["sa3"]).reshape(shape)
    m = good.copy()
    m[3] = good[4]
    out["one board's rows from its neighbour"] = m
    rows = good.reshape(n * 20, C).copy()
    last = (n * 20) // 16 * 16
    assert last < n * 20                                     # the last 16-row tile is ragged
    rows[last:-1] = good.reshape(n * 20, C)[last + 1:]
    out["the last ragged 16-row tile's rows shifted by one"] = rows.reshape(shape)
    return good, out


@pytest.mark.parametrize("C", [128, 512])
def test_wrong_conv3_kernels_leave_their_intervals(states, C):
    """Each mutant breaks the per-element interval somewhere (printed: the share of elements it breaks); the honest kernel it is
    derived from breaks none.  "sa2 used for sa3" needs parameters on which the two differ: C = 128 (32 and 64)."""
    r = rnd(states, C)
    n = N_MUTANT
    lo, hi = L8.accepted_codes(r["y3"][:n], r["beta3"][:n], r["sa3"])
    good, mutants = conv3_mutants(r, C, n)
    assert L8.inside(good, lo, hi).all()
    if C == 128:
        assert r["sa2"] != r["sa3"] and "sa2 used for sa3" in mutants
    for name, got in mutants.items():
        broken = float((~L8.inside(got, lo, hi)).mean())
        print(f"C {C} conv3, {name}: {broken:.4f} of the elements outside their interval")
        assert broken > 0, name


def test_wrong_conv4_kernels_leave_the_bound(states):
    """The same mutants on conv4 (bf16 output, |dev - relu(y)| <= 2^-8 relu(y) + beta) at C = 128."""
    C, n = 128, N_MUTANT
    r = rnd(states, C)
    qw, dq, b, _ = r["q"]["conv4"]
    A = L8.im2col("conv4", L8.code_values(r["codes3"][:n]))
    y, bound = np.maximum(r["y4"][:n], 0.0).reshape(-1, C), L8.conv4_bound(r["y4"][:n], r["beta4"][:n]).reshape(-1, C)
    fin = lambda acc, dq_=dq, b_=b: L.bf16_round64(L8.epilogue_f32(acc, dq_, b_))
    good_acc = L8.acc_blocks_f32(A, qw, C)
    good = fin(good_acc)
    assert (np.abs(good - y) <= bound).all()
    W2 = qw.copy()
    W2[2 * C:3 * C], W2[5 * C:6 * C] = qw[5 * C:6 * C], qw[2 * C:3 * C]
    A2 = A.copy().reshape(A.shape[0], -1, 8, 16)
    A2[:, :, [1, 5]] = A2[:, :, [5, 1]]
    trunc = L.bf16_from_bits((L8.epilogue_f32(good_acc, dq, b).view(np.uint32) >> 16).astype(np.uint16))
    board = good.reshape(n, 6, C).copy()
    board[3] = good.reshape(n, 6, C)[4]
    ragged = good.copy()
    last = (n * 6) // 16 * 16
    assert last < n * 6
    ragged[last:-1] = good[last + 1:]
    mutants = {"one dropped K-step": fin(L8.acc_blocks_f32(A, qw, C, skip=(4, 0))), "two taps swapped": fin(L8.acc_blocks_f32(A, W2, C)),
               "16-byte chunks 1 and 5 swapped in the activations only": fin(L8.acc_blocks_f32(A2.reshape(A.shape), qw, C)),
               "channel n with channel n + 1's dq": fin(good_acc, dq_=np.roll(dq, -1)), "channel n with channel n + 1's bias": fin(good_acc, b_=np.roll(b, -1)),
               "truncation in place of round-to-nearest-even": trunc, "one board's rows from its neighbour": board.reshape(-1, C),
               "the last ragged 16-row tile's rows shifted by one": ragged}
    for name, got in mutants.items():
        broken = float((np.abs(got - y) > bound).mean())
        print(f"C {C} conv4, {name}: {broken:.4f} of the elements over the bound")
        assert broken > 0, name


@pytest.mark.parametrize("C", [128, 512])
def test_conv2_is_exact_and_its_mutants_change_bits(states, C):
    """conv2_codes_ref is deterministic (the same rows, the same codes); an out-of-board tap that reads a real row (pattern 0's, the
    empty neighbourhood) instead of the zero row changes codes, and only at positions that have such a tap; two taps reading each
    other's table column change codes.

    The taps added in REVERSE ORDER do not change a single code, on any of the 150 boards at either width (806400 / 3225600
    elements), and cannot be expected to: an f16 entry has 11 significant bits, so the sum of nine of them fits f32's 24 bits unless
    the entries' exponents spread over more than 13 binary orders -- the f32 sum is the EXACT sum, whatever the order (asserted below:
    both orders equal the float64 sum in more than 0.999 of the elements; printed: the share).  The order of k_conv2_table_x8's adds is
    therefore not something its codes depend on at these magnitudes; what the bit-for-bit comparison of the GPU test pins is the
    gather (which row, which column, which positions), the bias, the scale and the conversion."""
    r = rnd(states, C)
    st = states[:N_MUTANT]
    good, _ = L8.conv2_codes_ref(r["U_of"], st, r["folded"], r["sa2"])
    assert np.array_equal(good, r["codes2"][:N_MUTANT])
    row0 = L.f16_bits(L.u_ref(r["T"][:1], r["folded"])[0])[0]
    assert row0.any()
    out, _ = L8.conv2_codes_ref(r["U_of"], st, r["folded"], r["sa2"], outside=row0)
    swap, _ = L8.conv2_codes_ref(r["U_of"], st, r["folded"], r["sa2"], rows_tap=[0, 1, 5, 3, 4, 2, 6, 7, 8])
    rev, _ = L8.conv2_codes_ref(r["U_of"], st, r["folded"], r["sa2"], order=range(8, -1, -1))
    exact = L8.conv2_sums(r["U_of"], st, dtype=np.float64)
    fwd32, rev32 = L8.conv2_sums(r["U_of"], st), L8.conv2_sums(r["U_of"], st, order=range(8, -1, -1))
    print(f"C {C} conv2: an out-of-board tap from a real row {float((out != good).mean()):.4f} of the codes differ; two taps' columns swapped "
          f"{float((swap != good).mean()):.4f}; taps in reverse order {int((rev != good).sum())} of {good.size} codes, {int((rev32 != fwd32).sum())} f32 sums; "
          f"f32 sums that are not the exact sum: {int((fwd32 != exact).sum())} in (ky, kx) order, {int((rev32 != exact).sum())} in reverse")
    assert (out != good).any() and (swap != good).any()
    assert (fwd32 == exact).mean() > 0.999 and (rev32 == exact).mean() > 0.999
    assert np.array_equal(rev[(fwd32 == exact) & (rev32 == exact)], good[(fwd32 == exact) & (rev32 == exact)])
    interior = np.zeros((6, 7), bool)
    interior[1:5, 1:6] = True
    assert np.array_equal(out[:, interior], good[:, interior])          # only positions with a tap outside the board can change


def test_accepted_codes_and_truncation():
    """The number formats of the reference: code_values is the e4m3 table, nearest_codes rounds to nearest even and is monotone,
    accepted_codes is the exact code for beta = 0, codes_truncated is the largest code not above the value."""
    v = L8.CODE_VALUES[:0x7F]
    assert v[0] == 0 and v[1] == 2.0 ** -9 and v[0x7E] == 448 and (np.diff(v) > 0).all()
    assert np.array_equal(L8.nearest_codes(v, 1.0), np.arange(0x7F, dtype=np.uint8))
    mid = (v[:-1] + v[1:]) / 2                                            # ties go to the even code
    tie = L8.nearest_codes(mid, 1.0)
    assert np.array_equal(tie, np.where(np.arange(0x7E) % 2 == 0, np.arange(0x7E), np.arange(0x7E) + 1).astype(np.uint8))
    assert np.array_equal(L8.codes_truncated(mid), np.arange(0x7E, dtype=np.uint8)) and np.array_equal(L8.codes_truncated(v), np.arange(0x7F, dtype=np.uint8))
    x = np.sort(np.random.default_rng(1).uniform(-2, 500, 4000))
    c = L8.nearest_codes(x, 1.0)
    assert (np.diff(c.astype(int)) >= 0).all() and c[0] == 0 and c[-1] == 0x7E
    lo, hi = L8.accepted_codes(x, np.zeros_like(x), 0.5)
    assert np.array_equal(lo, hi) and np.array_equal(lo, L8.nearest_codes(x / 2, 1.0))
    lo, hi = L8.accepted_codes(x, np.full_like(x, 0.3), 1.0)
    assert (lo <= c).all() and (c <= hi).all() and (lo < hi).any()
    assert L8.quantum(np.array([0.0, 6.0, 10.0])) == 1 and L8.quantum(np.array([0.375])) == -3 and L8.quantum(np.zeros(3)) is None


@pytest.mark.parametrize("channels", [128, 256, 384, 512])
def test_exact_data_conditions(states, channels):
    """What makes "bit for bit" a fair demand of the fp8 class, for the parameter seed, head shift and inputs of the GPU test: every
    layer's sum, in units of its operands' quanta, below 2^24 (any f32 order is exact), every layer alive, nothing saturated (codes or
    heads), the f32 evaluation of the reference equal to the float64 one, and an honest f32 kernel reproducing the stored codes."""
    params = exact_params(channels, L.EXACT_SEED, L8.HEAD_SHIFT[channels])
    sa2, sa3 = r8.calibrate_scales(params, L.boards_of(states), channels)
    out = L8.forward_exact(states, params, channels, sa2, sa3)
    L8.exact_conditions(out)
    out8 = L8.forward_exact(states[:8], params, channels, sa2, sa3, dtype=torch.float64)
    for name in ("act2", "act3", "act4", "fc1", "fc2"):
        assert np.array_equal(out8[name], out[name][:8]), name
    for name in ("conv3", "conv4"):
        assert np.array_equal(out8[name][0], out[name][0][:8]) and np.array_equal(out8[name][1], out[name][1][:8]), name
    q = L8.quantised(params, channels, sa2, sa3)
    qw, dq, b, _ = q["conv3"]
    got = L8.store_conv3(L8.epilogue_f32(L8.acc_blocks_f32(L8.im2col("conv3", L8.code_values(out["act2"][:4])), qw, channels), dq, b), sa3)
    assert np.array_equal(got.reshape(4, 4, 5, channels), out["act3"][:4])
    # the whole-net emulation of net_ref_fp8 stores the same conv3 codes and heads
    epi, ev, info = r8.forward_fp8(params, L.boards_of(states[:24]), channels, sa2, sa3, details=True)
    assert np.array_equal(info["act3_codes"], out["act3"][:24])
    assert np.abs(epi - out["pi"][:24]).max() <= 1e-6 and np.abs(ev - out["v"][:24]).max() <= 1e-6
    print(channels, "scales", sa2, sa3, "largest scaled activations", out["scaled_max"], "sums in quanta (max, bias a multiple)", out["units"],
          "distinct act3 codes", np.unique(out["act3"]).size, "nonzero", float((out["act3"] != 0).mean()), "pi", out["pi"].min(), out["pi"].max(),
          "|v|", np.abs(out["v"]).max())
