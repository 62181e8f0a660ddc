"""Layer-by-layer reference of the "net_fp8" numerics class in float64 on the CPU, with the bounds the fp8 layer tests hold the
kernels to (tests/test_net_layers_fp8_cpu.py, tests/test_net_layers_fp8_gpu.py).  Built on net_layers_ref.py (inputs, conv1, the
FCs, the heads, the bf16 bound) and net_ref_fp8.py (the fold, weight_scales, pow2_scale, the e4m3 conversions); layouts are the
engine's: channels-last, K index of a conv = tap * C + ci.

  conv2   k_conv2_table_x8 is reproducible EXACTLY: the nine f16 table entries added in (ky, kx) order into an f32 zero, + the f32
          bias, ReLU, * sa2, clamp to +-448, round to nearest even.  conv2_codes_ref does the same in numpy f32 from the table rows
          it is given: from the device's own u2 rows the codes must be the device's bit for bit, on random data too.
  conv3 / conv4   per output element, from e4m3 input codes a, weight codes qw = e4m3(w' sw[n]) and dq[n] = 1 / (sw[n] sa_in), in
          float64: acc = sum a qw, S = sum |a||qw|, y = acc dq + b, beta = (K + 1) 2^-23 (S dq + |b|) -- the worst case of ANY f32
          summation order of K exact products and a bias with truncating partial sums (bound_bf16's second term; the products of two
          e4m3 numbers are exact in f32, the multiplication by the power of two dq is exact).  Derived, not measured.
          conv3 stores e4m3 codes: rounding is monotone, so a device value inside [y - beta, y + beta] stores a code between
          e4m3(relu(y - beta) sa3) and e4m3(relu(y + beta) sa3) inclusive (accepted_codes); where the two coincide the element must
          be that exact code.  conv4 stores bf16: |dev - relu(y)| <= 2^-8 relu(y) + beta.
  exact data   integer parameters (net_ref.exact_params): every operand is a multiple of a power-of-two quantum and S in units of
          the quanta's product stays below 2^24, so every f32 order gives the exact sum and every stored value is a deterministic
          rounding of an exact number: act2 / act3 codes and act4 / fc1 / fc2 bf16 bits must be the reference's (forward_exact).

What the bound cannot see is stated by the non-vacuity conditions (nonvacuous): the share of conv3 elements with more than one
accepted code is capped (SHARE_CAP), the layer is alive and nothing saturates -- all from the reference alone.

Saturating activations are out of scope on the device: the activation scales come from the weights alone (a calibration set that is
a constant of the library) with 4 x headroom, so no legal input reaches +-448; tests/test_fp8_cpu.py covers the host quantiser's
clamp, and the conditions here assert that the test data stay clear of it.
"""
import numpy as np
import torch
import torch.nn.functional as F

import net_layers_ref as L
import net_ref_fp8 as r8
from net_ref import unpack

FP8_MAX = r8.FP8_MAX
CODE_VALUES = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()     # value of every code (0x7F / 0xFF: NaN)
SHARE_CAP = {128: 0.10, 512: 0.35}      # most conv3 elements with more than one accepted code (measured 0.0745 / 0.302 on the emulation's inputs)
# exact_params' head weights 2^-shift for the fp8 class: L.HEAD_SHIFT's 18 saturates the heads at 384 / 512 here (pi max 0.998 / 0.9999994)
HEAD_SHIFT = {128: 18, 256: 19, 384: 20, 512: 21}


# ---- number formats -------------------------------------------------------------------------------------------------
def code_values(codes):
    """uint8 e4m3 codes -> float64 values."""
    return CODE_VALUES[np.asarray(codes, np.uint8)]


def codes_of(x):
    """float array (already scaled) -> e4m3 codes: to f32, clamp to +-448, round to nearest even (the device's pack_fp8x4).  The
    composition float64 -> f32 -> e4m3 is monotone, which is all accepted_codes needs; an f32 input is converted as the device does."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32)
    return r8.e4m3_codes(t).numpy()


def codes_truncated(x):
    """... with the rounding replaced by truncation towards zero (a mutant: the largest code whose value is <= x), x >= 0."""
    x = np.minimum(np.asarray(x, np.float64), FP8_MAX)
    return (np.searchsorted(CODE_VALUES[:0x7F], x, side="right") - 1).astype(np.uint8)


def nearest_codes(y, scale):
    """The code an exact kernel stores for the unrounded pre-ReLU value y: e4m3(relu(y) * scale)."""
    return codes_of(np.maximum(np.asarray(y, np.float64), 0.0) * float(scale) + 0.0)


def accepted_codes(y, beta, scale):
    """(lo, hi) uint8: the codes a kernel within beta of y may store, inclusive, in value order (non-negative codes order like their
    values)."""
    return nearest_codes(y - beta, scale), nearest_codes(y + beta, scale)


def inside(codes, lo, hi):
    codes = np.asarray(codes, np.uint8)
    assert codes.shape == lo.shape == hi.shape, (codes.shape, lo.shape, hi.shape)            # no broadcasting: every element
    return (codes >= lo) & (codes <= hi)


def quantum(x):
    """The largest power of two (as an exponent) that divides every element of x (dyadic rationals); None for an all-zero x."""
    u = np.unique(np.abs(np.asarray(x, np.float64)))
    u = u[u != 0]
    if u.size == 0:
        return None
    for k in range(40, -60, -1):
        s = np.ldexp(u, -k)
        if np.array_equal(s, np.rint(s)):
            return k
    raise AssertionError("not dyadic")


# ---- conv2: the table gather, exactly ---------------------------------------------------------------------------------
def conv2_sums(U_of, states, order=range(9), outside=None, rows_tap=range(9), dtype=np.float32):
    """The gather's sum over the nine taps, before the bias: [n][6][7][C] in `dtype`, the taps added in `order` into a zero.
    U_of(patterns) -> the table rows [len(patterns)][9][C] as f16 BITS (uint16) for an int array of pattern indices.
    outside / rows_tap are the mutants' handles: a [9][C] f16-bits row that out-of-board taps read instead of the appended zero row, and
    the table column tap t reads (the identity in the kernel).  dtype = np.float64 gives the exact sum."""
    pat = L.patterns_of(states)
    n = pat.shape[0]
    uniq, inv = np.unique(pat, return_inverse=True)
    rows = np.ascontiguousarray(U_of(uniq), dtype=np.uint16).view(np.float16)           # [u][9][C]
    inv = inv.reshape(n, 6, 7)
    C = rows.shape[-1]
    acc = np.zeros((n, 6, 7, C), dtype)
    for t in order:
        ky, kx = divmod(t, 3)
        y0, y1, x0, x1 = max(0, 1 - ky), min(6, 7 - ky), max(0, 1 - kx), min(7, 8 - kx)      # outputs whose neighbour is on the board
        g = np.zeros((n, 6, 7, C), dtype)                       # the zero row: + 0, as the kernel adds it
        if outside is not None:
            g[:] = np.ascontiguousarray(outside, dtype=np.uint16).view(np.float16)[t].astype(dtype)
        g[:, y0:y1, x0:x1] = rows[:, rows_tap[t]][inv[:, y0 + ky - 1:y1 + ky - 1, x0 + kx - 1:x1 + kx - 1]].astype(dtype)
        acc += g
    assert acc.dtype == dtype
    return acc


def conv2_codes_ref(U_of, states, folded, sa2, **mutant):
    """k_conv2_table_x8 operation for operation: conv2_sums in f32 in (ky, kx) order, + the f32 bias, ReLU, * sa2, clamp, round to
    nearest even -> (codes [n][6][7][C] uint8, the largest scaled activation before the clamp)."""
    acc = conv2_sums(U_of, states, **mutant)
    scaled = np.maximum(acc + np.asarray(folded["conv2"][1], np.float32), np.float32(0)) * np.float32(sa2)
    assert scaled.dtype == np.float32
    return codes_of(scaled), float(scaled.max())


# ---- conv3 / conv4 ------------------------------------------------------------------------------------------------------
def quantised(params, C, sa2, sa3):
    """{"conv3" / "conv4": (qw [9C][C] float64 values of the weight codes, dq [C], b [C], sw [C])}: the f32 fold of net_ref_fp8, the
    per-output-channel power-of-two scale, the weights as e4m3(w' * sw[n]) and dq[n] = 1 / (sw[n] * sa_in) in f32."""
    P = unpack(np.asarray(params, np.float32), C)
    out = {}
    for name, sa_in in (("conv3", sa2), ("conv4", sa3)):
        wf, bf = r8._fold(P[name + "_w"], P[name + "_b"], P[name + "_bn"])
        sw = r8.weight_scales(wf)
        qw = r8.e4m3(wf * sw).reshape(9 * C, C)
        dq = (1.0 / (sw * np.float32(sa_in))).to(torch.float32)
        assert wf.dtype == torch.float32 and dq.dtype == torch.float32
        out[name] = (qw.double().numpy(), dq.double().numpy(), bf.double().numpy(), sw.double().numpy())
    return out


def layer8_ref(name, a, q, dtype=torch.float64):
    """conv3 / conv4 from ITS OWN input (a [n][h][w][C]: float64 values of e4m3 codes) -> (y unrounded and before the ReLU, beta, T) in
    float64 with T = S dq + |b|.  dtype = torch.float32 computes the sums in f32 (exact data: equal to float64)."""
    qw, dq, b, _ = q[name]
    K = qw.shape[0]
    acc = L._gemm_form(name, a, qw, dtype).to(torch.float64).numpy()
    S = L._gemm_form(name, np.abs(a), np.abs(qw), dtype).to(torch.float64).numpy()
    T = S * dq + np.abs(b)
    return acc * dq + b, (K + 1) * 2.0 ** -23 * T, T


def conv4_bound(y, beta):
    """|dev - relu(y)| <= 2^-8 relu(y) + beta: bound_bf16 with T in the place of S."""
    return 2.0 ** -8 * np.maximum(y, 0.0) + beta


def nonvacuous(y, beta, sa3, cap):
    """The conditions under which conv3's interval test means something, from the reference alone -> (share of elements with more
    than one accepted code, share with more than two, share of nonzero nearest codes)."""
    lo, hi = accepted_codes(y, beta, sa3)
    near = nearest_codes(y, sa3)
    share, share2, alive = float((lo != hi).mean()), float((hi.astype(int) - lo > 1).mean()), float((near != 0).mean())
    assert share <= cap, (share, cap)
    assert alive > 0.1, alive
    assert (np.maximum(y + beta, 0.0) * sa3).max() < FP8_MAX                    # nothing saturates
    return share, share2, alive


# ---- honest f32 kernels (the CPU test's twins, and the GPU test's yardstick for "codes off the nearest one") ----------------
def im2col(name, a):
    """[M][K] float64 with K = tap * C + ci ('valid' 3 x 3)."""
    a = np.asarray(a, np.float64)
    n, h, w, c = a.shape
    return np.concatenate([a[:, ky:ky + h - 2, kx:kx + w - 2].reshape(-1, c) for ky in range(3) for kx in range(3)], axis=1)


def engine_k_order(C):
    """The K-steps (tap, first channel) in the engine's order: channel block outer, tap inner."""
    return [(t, c0) for c0 in range(0, C, 128) for t in range(9)]


def acc_blocks_f32(A, W, C, skip=None):
    """The MFMA's shape: every K-step's 128 products summed exactly (float64: they are exact and their sum fits), the steps
    accumulated in f32 in the engine's order.  skip = a (tap, c0) step left out (a mutant)."""
    acc = np.zeros((A.shape[0], W.shape[1]), np.float32)
    for t, c0 in engine_k_order(C):
        if (t, c0) == skip:
            continue
        k = slice(t * C + c0, t * C + c0 + 128)
        acc = (acc.astype(np.float64) + A[:, k] @ W[k]).astype(np.float32)
    return acc


def acc_sequential_f32(A, W, C):
    """One product at a time in f32, in the engine's K order."""
    A32, W32 = A.astype(np.float32), W.astype(np.float32)
    acc = np.zeros((A.shape[0], W.shape[1]), np.float32)
    for t, c0 in engine_k_order(C):
        for k in range(t * C + c0, t * C + c0 + 128):
            acc += A32[:, k:k + 1] * W32[k]
    return acc


def acc_torch_f32(a, qw):
    """torch's own f32 convolution (its order is its own)."""
    C = a.shape[-1]
    x = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).permute(0, 3, 1, 2).contiguous()
    w = torch.from_numpy(qw).to(torch.float32).reshape(3, 3, C, -1).permute(3, 2, 0, 1).contiguous()
    return F.conv2d(x, w).permute(0, 2, 3, 1).reshape(-1, w.shape[0]).numpy()


def epilogue_f32(acc, dq, b):
    """The kernels' epilogue in f32: acc * dq + b, ReLU -> [M][N] f32."""
    r = (np.asarray(acc, np.float32) * dq.astype(np.float32) + b.astype(np.float32)).astype(np.float32)
    return np.maximum(r, np.float32(0))


def store_conv3(r, sa3):
    return codes_of(np.asarray(r, np.float32) * np.float32(sa3))


def off_nearest(codes, near):
    """(elements whose code is not the nearest one, how many of those are exactly one step away)."""
    d = np.asarray(codes, np.uint8).astype(int) - np.asarray(near, np.uint8).astype(int)
    return int((d != 0).sum()), int((np.abs(d) == 1).sum())


# ---- the whole exact forward ----------------------------------------------------------------------------------------
def forward_exact(states, params, C, sa2, sa3, dtype=torch.float32, conv1=None):
    """exact_params through the fp8 class, every layer from the stored form of the one before -> {"act2", "act3": codes, "act4",
    "fc1", "fc2": bf16 bits, "pi", "v", and what exact_conditions reads}.  conv2 is the GEMM form's sum: on exact data the table
    entries are exact integers of at most 2048, so the table gather adds the same numbers (net_layers_ref's exact-data conditions).
    conv1 = net_layers_ref.conv1_from_table's pair takes the place of conv1_ref on every board."""
    folded = L.fold_like_engine(params, C)
    q = quantised(params, C, sa2, sa3)
    y1, S1 = L.conv1_ref(states, folded) if conv1 is None else conv1
    y2, S2 = L.layer_ref("conv2", L.bf16_round64(y1), folded, dtype)
    out = {"S1": float(np.max(S1)), "conv2": (y2, S2), "act2": nearest_codes(y2, sa2), "scaled_max": [float(y2.max() * sa2)], "units": {}}
    a = code_values(out["act2"])
    for name in ("conv3", "conv4"):
        y, beta, T = layer8_ref(name, a, q, dtype)
        qw, dq, b, _ = q[name]
        ka, kw, kd = quantum(a), quantum(qw), quantum(dq)
        assert ka is not None and kw is not None and np.array_equal(dq, np.exp2(np.round(np.log2(dq))))
        unit = 2.0 ** (ka + kw) * dq                      # per output channel: every product times dq is a multiple of it
        out["units"][name] = (float((T / unit).max()), bool(np.array_equal(b / unit, np.rint(b / unit))))
        out[name] = (y, T)
        if name == "conv3":
            out["act3"] = nearest_codes(y, sa3)
            out["scaled_max"].append(float(np.maximum(y, 0).max() * sa3))
            a = code_values(out["act3"])
        else:
            out["act4"] = L.bf16_bits(np.maximum(y, 0.0))
            a = L.bf16_from_bits(out["act4"])
    for name in ("fc1", "fc2"):
        y, S = L.layer_ref(name, a, folded, dtype)
        out[name + "_yS"] = (y, S)
        out[name] = L.bf16_bits(y)
        a = L.bf16_from_bits(out[name])
    out["pi"], out["v"], _ = L.heads_ref(a, folded)
    return out


def exact_conditions(out):
    """What makes "bit for bit" a fair demand of forward_exact's result, from the reference alone."""
    assert out["S1"] < 2 ** 24
    y2, S2 = out["conv2"]
    assert S2.max() < 2 ** 24 and np.array_equal(y2, np.rint(y2))
    for name in ("conv3", "conv4"):
        units, bias_ok = out["units"][name]
        assert units < 2 ** 24 and bias_ok, (name, units, bias_ok)             # every f32 order of the layer's sum is exact
    for name in ("fc1", "fc2"):
        y, S = out[name + "_yS"]
        assert S.max() < 2 ** 24 and np.array_equal(y, np.rint(y)), name
    assert max(out["scaled_max"]) < FP8_MAX                                     # nothing saturates
    for name in ("act2", "act3"):
        assert np.unique(out[name]).size > 16 and (out[name] != 0).mean() > 0.1, name
    for name in ("act4", "fc1", "fc2"):
        assert np.unique(out[name]).size > 16 and (out[name] != 0).mean() > 0.1, name
    assert out["pi"].max() < 0.999 and np.abs(out["v"]).max() < 0.999            # no saturated head that could hide a difference
