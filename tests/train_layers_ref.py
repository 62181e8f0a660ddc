"""Kernel-by-kernel float64 reference of ONE training step (csrc/az_train.hip), with the per-element error bound each kernel is held
to (tests/test_train_layers_cpu.py, tests/test_train_layers_gpu.py).

Teacher forcing: every function takes what the DEVICE fed to one kernel (read back through the diagnostic library's az_diag_train_read)
and returns that kernel's exact output y in float64 plus the bound on |dev - y|.  Errors do not compound through the layers and a ReLU
never flips, so every bound sits at rounding level and a failure names its kernel.  Every element of every tensor is compared.

Layouts are the trainer's: activations channels-last ([b][h][w][C] = rows x C), K index of a conv GEMM = tap * Cin + ci with
tap = ky * 3 + kx, fc1's input = conv4's [b][2][3][C] flattened, layer l = 0..5 is conv1..conv4, fc1, fc2.

THE BOUNDS ARE DERIVED, NOT MEASURED.  u = 2^-24 is f32's unit roundoff (round to nearest: the VALU kernels); the matrix cores' adders
are given 2 u = 2^-23 per addition (nearest or truncating, whatever their internal order).

  GEMMs        out = sum_k a_k w_k (+ bias), K products, S = sum |a_k| |w_k| (+ |bias|):       |dev - y| <= e_fmt + n_acc 2^-23 S
               (split-K slices start from 0 and are added in f32: they reorder the same additions; col2im's nine f32 additions and the
               bias count as terms).  Per operand format (gemm_format says which GEMM of which GEMM set uses which):
    f32        k_gemm_f32 / k_gemm_f32_dma, v_mfma_f32_16x16x4_f32: operands exact, every product rounded once, K - 1 additions, the
               bias: e_fmt = 0, n_acc = K + 1.  This is the (K + 1) 2^-23 S of tests/net_layers_ref.py.
    bf16 x 3   k_gemm3 / k_gemm3_ring / k_wgrad3_tr: x -> hi = bf16(x), lo = bf16(x - hi).  bf16 keeps 8 significand bits (unit roundoff
               2^-8), so |x - hi| <= 2^-8 |x| and |x - hi - lo| <= 2^-16 |x|.  hi hi + hi lo + lo hi leaves out a_lo w_lo
               (<= 2^-16 |a w|) and the two operands' residuals (2^-16 |a w| each, to first order): e_fmt = 3 x 2^-16 (1 + 2^-7) S.
               The three products are exact in f32 (8 + 8 bits) and of total size <= (1 + 2^-5) |a w|; 3 K terms are accumulated:
               n_acc = (3 K + 1)(1 + 2^-5).
    f16 x 3    the conv2..conv4 forward: the operands are s_l a and 256 W (powers of two: exact), split in IEEE half (11 bits:
               residual 2^-22 |x|) -- but the matrix cores flush half subnormals, so a hi or lo below 2^-14 is lost: the residual of an
               operand x' is <= 2^-22 |x'| + 2^-14 in scaled units, i.e. 2^-22 |a| + 2^-14 / s_l and 2^-22 |w| + 2^-22 unscaled.
               e_fmt = 3 x 2^-22 (1 + 2^-9) S + 2^-22 sum|a_k| + (2^-14 / s_l) sum|w_k|; products of two 11-bit numbers are exact in
               f32; n_acc as for bf16 x 3.  s_l is act_scales_body's, recomputed here; the reference ASSERTS that s_l a and 256 W are
               finite in half precision (the range contract of the f16 forward).
               The final multiplication by 1 / (256 s_l) is by a power of two, the bias addition is one of the n_acc terms.
    What these bounds can and cannot see: n_acc 2^-23 is a worst case over summation orders, and it grows with K where honest errors
    grow with sqrt(K).  A lost K-step, row block, tap, transposed block or wrong row is O(S / K) .. O(S) and is seen at every K; a lost
    cross term (2^-8 or 2^-11 of each product at most, random signs) is seen while K is a few hundred (the dgrads at C = 128, the FC and small
    batch wgrads), not under the 1152 .. 4608 products of the wider forward GEMMs.  tests/test_train_layers_cpu.py shows both.

  BatchNorm forward (k_colreduce<0> + k_bn_apply, k_bn_fwd_small): column sums of z and z^2 in DOUBLE partials (M additions of
               exactly converted f32 values, 2^-53 each), mu = sum / M, var = E[z^2] - mu^2 in double, then one f32 rounding each:
      mean     E_mean = u |mu| + (M + 2) 2^-53 sum|z| / M
      var      E_var  = (3 M + 8) 2^-53 E[z^2]                    (E[z^2] - mu^2 in double: M 2^-53 E[z^2] from the sum of squares and
               2 |mu| x the mean's M 2^-53 mean|z| <= 2 M 2^-53 E[z^2] by Cauchy-Schwarz, the divisions and the subtraction)
      invstd   E_inv  = u inv + inv^3 E_var / 2 + 2^-50 inv       (d inv / d var = - inv^3 / 2; double sqrt and division)
      a        y = gamma ((z - mean) inv) + beta is three f32 operations on xhat's path and one addition:
               E_y = |gamma| inv E_mean + |gamma| |z - mean| E_inv + u (3 |gamma xhat| + |y|); ReLU is 1-Lipschitz; a kept dropout
               element is multiplied by the f32 1 / keep: + u |a|; a dropped one is exactly 0.
      moving   r = m r0 + (1 - m) x in f32 (m = 0.99f, 1 - m computed in f32): u (|m r0| + |(1 - m) x| + |r|) + (1 - m) E_x, with
               x = mean, or the unbiased variance var M / (M - 1) (one more rounding: + u |(1 - m) x|).
  BatchNorm backward (k_colreduce<1> + k_bn_bwd_apply, k_bn_bwd_small): inputs d loss / d a (go), z, the stored mean / invstd, and the
               ReLU mask the kernel RECOMPUTES as gamma ((z - mean) invstd) + beta > 0 in f32 (bn_grad_in; it does not read a[l]).
               g = go on the kept side of ReLU and dropout (x the f32 1 / keep: u |g| with dropout), xhat rounded twice (2 u).
      dbeta    sum g in double partials, one f32 rounding:     E_b = u |dbeta| + (u_drop + (M + 2) 2^-53) sum|g|
      dgamma   sum g xhat, product in double:                  E_g = u |dgamma| + (2 u + u_drop + (M + 2) 2^-53) sum|g xhat|
      dz       gamma invstd (g - (dbeta + xhat dgamma) / M) in f32 -- operation by operation (xhat 2, the product 1, the sum 1, the
               multiplication by the rounded 1 / M 2, the subtraction 1, gamma invstd and the last product 2):
               E_dz = |gamma invstd| (u (4 |g| + 6 |dbeta| / M + 9 |xhat dgamma| / M) + (E_b + |xhat| E_g) / M)
      mask     an element whose float64 pre-activation lies within u (3 |gamma xhat| + |y|) of zero may be cut on either side; they are
               counted, at most MASK_CAP per layer are allowed, and a column that has one is accepted if ANY choice of its ambiguous
               elements meets the bounds (the columns of a BatchNorm backward are independent).
      Pre-BatchNorm bias gradients are exactly 0 (the kernels never write them).
  Heads (k_heads_loss, k_heads_bwd): f32 VALU dot products, (K + 1) u S.  The softmax / loss stage is checked from the logits and v
               the DEVICE stored (they are what the kernel's own second half reads), with expf / logf / tanhf taken at the OpenCL
               full-profile limits OCML implements (3, 3 and 5 ulp; 1 ulp = 2^-23 relative); heads_stage2 spells the propagation out.

Second-order terms are covered by SEC = (1 + u)^32 on every VALU bound.
"""
import numpy as np
import torch
import torch.nn.functional as F

from net_ref import layout
from train_ref import dropout_mask

U = 2.0 ** -24
U_MFMA = 2.0 ** -23
SEC = (1.0 + U) ** 32
ULP = 2.0 ** -23
ULP_EXP, ULP_LOG, ULP_TANH = 3, 3, 5
BN_EPS = float(np.float32(1e-3))
MOM = float(np.float32(0.99))
ONE_MINUS_MOM = float(np.float32(1.0) - np.float32(0.99))
MASK_CAP = 4

NAMES = ("conv1", "conv2", "conv3", "conv4", "fc1", "fc2")
GEO = ((6, 7, 1), (6, 7, 1), (6, 7, 0), (4, 5, 0))          # conv layer l: input H, W, pad
ROWS_PER = (42, 42, 20, 6, 1, 1)

# az_train.h TrainDiagBuf
Z, A, MEAN, INVSTD, LOGITS, DHEAD, LOSS, KEPT_DACT, KEPT_DZ = range(9)


def n_out(C):
    return (C, C, C, C, 1024, 512)


def unpack64(p, C):
    """flat f32 parameters -> {name: float64 array in its layout() shape}."""
    return {k: np.asarray(p[o:o + int(np.prod(shp))], np.float64).reshape(shp) for k, (o, shp) in layout(C)[0].items()}


# ---- the reader's ctypes wrapper -------------------------------------------------------------------------------------
def read_shape(what, layer, rows, C):
    """Shape of buffer `what` of `layer` for `rows` samples; ValueError for what the library would refuse without being asked."""
    if what not in range(9):
        raise ValueError(f"no such buffer {what}")
    if not isinstance(rows, (int, np.integer)) or rows <= 0 or rows > 256:
        raise ValueError(f"rows {rows} outside [1, 256]")
    if C < 128 or C % 128:
        raise ValueError(f"width {C}")
    if what in (LOGITS, DHEAD):
        return (rows, 8)
    if what == LOSS:
        return (rows, 2)
    if not isinstance(layer, (int, np.integer)) or layer < 0 or layer > 5:
        raise ValueError(f"no such layer {layer}")
    if what in (MEAN, INVSTD):
        return (n_out(C)[layer],)
    return (rows * ROWS_PER[layer], n_out(C)[layer])


def read(e, what, layer, rows, C):
    """Buffer `what` of the engine's trainer after a step -> float32 array (read_shape).  RuntimeError if the library refuses."""
    import ctypes
    shape = read_shape(what, layer, rows, C)
    f = e._lib.az_diag_train_read
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    out = np.empty(shape, np.float32)
    got = f(e._h, int(what), int(layer), int(rows), out.ctypes.data_as(ctypes.c_void_p))
    if got != out.nbytes:
        raise RuntimeError(f"az_diag_train_read({what}, {layer}, {rows}) -> {got}, expected {out.nbytes}")
    return out


def refuses(e, what, layer, rows):
    """The raw call answers -1 (nothing is copied: a small buffer will do)."""
    import ctypes
    f = e._lib.az_diag_train_read
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return f(e._h, int(what), int(layer), int(rows), np.empty(16, np.float32).ctypes.data_as(ctypes.c_void_p)) == -1


def set_keep(e, on):
    """az_diag_train_keep -> True if accepted."""
    import ctypes
    f = e._lib.az_diag_train_keep
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return f(e._h, int(on)) == 0


# ---- number formats --------------------------------------------------------------------------------------------------
def split_bf16(x):
    """f32 array -> (hi, lo) as float32: hi = bf16(x), lo = bf16(x - hi), round to nearest even (az_train.hip split_bf16)."""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi.numpy(), lo.numpy()


def split_f16(x):
    """The same in IEEE half, with the matrix cores' flush of half subnormals applied to both parts (split_f16 + mfma)."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(over="ignore"):
        hi = x.astype(np.float16).astype(np.float32)
        lo = (x - hi).astype(np.float16).astype(np.float32)
    tiny = np.float32(2.0 ** -14)
    return np.where(np.abs(hi) < tiny, np.float32(0), hi), np.where(np.abs(lo) < tiny, np.float32(0), lo)


def act_scale(gamma, beta, rows):
    """act_scales_body: the power of two s_l <= 64 with s_l (max |gamma| sqrt(rows - 1) + max(beta, 0)) < 2^15, in f32."""
    sq = np.float32(np.sqrt(float(rows - 1)))
    bmax = np.max(np.abs(np.asarray(gamma, np.float32)) * sq + np.maximum(np.asarray(beta, np.float32), np.float32(0)))
    sc = np.float32(64.0)
    while sc > np.float32(2.0 ** -24) and not (sc * bmax < np.float32(32768.0)):
        sc = sc * np.float32(0.5)
    return float(sc)


def gemm_format(kind, l, gemm_set):
    """Operand format of layer l's GEMM `kind` ("fwd", "wgrad", "dgrad") under gemm_set = (train_gemm, train_fwd_dma, train_fwd_x3),
    as enqueue_step chooses it: conv1 and the FC forwards always on the f32 cores, conv2..conv4's forward as f16 x 3 when both
    train_gemm and train_fwd_x3 are on, every backward GEMM above conv1 as bf16 x 3 when train_gemm is on."""
    x3 = gemm_set[0] == 1
    if kind == "fwd":
        return "f16x3" if x3 and gemm_set[2] == 1 and 1 <= l <= 3 else "f32"
    return "bf16x3" if x3 and l >= 1 else "f32"


def gemm_bound(fmt, K, S, sum_a=None, sum_w=None, s_act=None):
    """The GEMM bound of the module docstring for K products of total magnitude S (arrays broadcast)."""
    if fmt == "f32":
        return (K + 1) * U_MFMA * S
    n_acc = (3 * K + 1) * (1 + 2.0 ** -5)
    if fmt == "bf16x3":
        return (3 * 2.0 ** -16 * (1 + 2.0 ** -7) + n_acc * U_MFMA) * S
    assert fmt == "f16x3" and s_act is not None
    return (3 * 2.0 ** -22 * (1 + 2.0 ** -9) + n_acc * U_MFMA) * S + 2.0 ** -22 * sum_a + (2.0 ** -14 / s_act) * sum_w


def ratio(dev, y, bound):
    """max over EVERY element of |dev - y| / bound; where the bound is 0 the device must be exact."""
    dev = np.asarray(dev, np.float64)
    assert dev.shape == y.shape == np.broadcast_to(bound, y.shape).shape, (dev.shape, y.shape)
    assert np.isfinite(dev).all() and np.isfinite(y).all()
    err = np.abs(dev - y)
    bound = np.broadcast_to(bound, y.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


# ---- the GEMMs --------------------------------------------------------------------------------------------------------
def _nhwc(l, a_in, C):
    """Layer l's input as [b][H][W][Cin] float64: the boards for conv1, else the previous layer's rows."""
    H, W, _ = GEO[l]
    if l == 0:
        return np.asarray(a_in, np.float64).reshape(-1, 2, 6, 7).transpose(0, 2, 3, 1)
    return np.asarray(a_in, np.float64).reshape(-1, H, W, C)


def fwd_gemm(l, C, a_in, P, fmt="f32"):
    """z[l] from the layer's device input (boards [b][2][6][7] for l = 0, else a[l-1] as read) -> (y, bound), both [rows][N].
    Conv layers are computed as convolutions (torch conv2d in float64): im2col, the gather and the tap order are under test."""
    w, bias = P[NAMES[l] + "_w"], P[NAMES[l] + "_b"]
    if l >= 4:
        a = np.asarray(a_in, np.float64).reshape(-1, w.shape[0])
        y = a @ w + bias
        S = np.abs(a) @ np.abs(w) + np.abs(bias)
        return y, gemm_bound("f32", w.shape[0], S)
    pad = GEO[l][2]
    x = torch.from_numpy(np.ascontiguousarray(_nhwc(l, a_in, C).transpose(0, 3, 1, 2)))
    wt = torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1)))

    def conv(xx, ww, bb):
        out = F.conv2d(xx, ww, bb, padding=pad)
        return out.permute(0, 2, 3, 1).reshape(-1, out.shape[1]).numpy()
    y = conv(x, wt, torch.from_numpy(bias.copy()))
    S = conv(x.abs(), wt.abs(), torch.from_numpy(np.abs(bias)))
    K = 9 * w.shape[2]
    if fmt != "f16x3":
        return y, gemm_bound(fmt, K, S)
    bn = P[NAMES[l - 1] + "_bn"]
    s = act_scale(bn[0], bn[1], x.shape[0] * ROWS_PER[l - 1])
    assert float(x.abs().max()) * s < 65504.0 and np.abs(w).max() * 256.0 < 65504.0, "f16 x 3 range contract"
    sum_a = conv(x.abs(), torch.ones_like(wt[:1]), None)                 # [rows][1]: the window's sum |a|
    sum_w = np.abs(w).reshape(-1, w.shape[3]).sum(axis=0)               # [N]: all nine taps (>= the taps inside the map)
    return y, gemm_bound(fmt, K, S, sum_a, sum_w[None, :], s)


def _windows(l, x):
    """(ky, kx, window) of layer l's padded input x [b][H][W][Cin]: window [b][Ho][Wo][Cin] = the input cell tap (ky, kx) reads."""
    H, W, pad = GEO[l]
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    xp = np.zeros((x.shape[0], H + 2 * pad, W + 2 * pad, x.shape[3]))
    xp[:, pad:pad + H, pad:pad + W] = x
    for ky in range(3):
        for kx in range(3):
            yield ky, kx, xp[:, ky:ky + Ho, kx:kx + Wo]


def wgrad(l, C, a_in, dz, fmt="f32"):
    """d loss / d W of layer l = (input)^T dz from the device input and the kept dz[l] -> (y, bound) in the weight's layout() shape,
    flattened.  The contraction runs over the rows: K = rows."""
    dz = np.asarray(dz, np.float64)
    M = dz.shape[0]
    if l >= 4:
        a = np.asarray(a_in, np.float64).reshape(M, -1)
        return (a.T @ dz).reshape(-1), gemm_bound(fmt, M, np.abs(a).T @ np.abs(dz)).reshape(-1)
    x = _nhwc(l, a_in, C)
    y = np.zeros((3, 3, x.shape[3], dz.shape[1]))
    S = np.zeros_like(y)
    for ky, kx, win in _windows(l, x):
        col = win.reshape(M, -1)
        y[ky, kx] = col.T @ dz
        S[ky, kx] = np.abs(col).T @ np.abs(dz)
    return y.reshape(-1), gemm_bound(fmt, M, S).reshape(-1)


def dgrad(l, C, dz, P, fmt="f32"):
    """d loss / d a[l-1] = dz W^T (+ col2im for a conv, or the gathered transposed convolution) from the kept dz[l] -> (y, bound),
    [rows of l-1][N of l-1].  K = N per tap; a conv adds its (at most) nine taps in f32: K = 9 N + 9."""
    dz = np.asarray(dz, np.float64)
    w = P[NAMES[l] + "_w"]
    if l >= 4:
        return dz @ w.T, gemm_bound(fmt, w.shape[1], np.abs(dz) @ np.abs(w).T)
    H, W, pad = GEO[l]
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    b, N = dz.shape[0] // (Ho * Wo), dz.shape[1]
    y = np.zeros((b, H + 2 * pad, W + 2 * pad, w.shape[2]))
    S = np.zeros_like(y)
    for ky in range(3):
        for kx in range(3):
            y[:, ky:ky + Ho, kx:kx + Wo] += (dz @ w[ky, kx].T).reshape(b, Ho, Wo, -1)
            S[:, ky:ky + Ho, kx:kx + Wo] += (np.abs(dz) @ np.abs(w[ky, kx]).T).reshape(b, Ho, Wo, -1)
    y, S = (t[:, pad:pad + H, pad:pad + W].reshape(b * H * W, -1) for t in (y, S))
    return y, gemm_bound(fmt, 9 * N + 9, S)


# ---- BatchNorm --------------------------------------------------------------------------------------------------------
def drop_of(mask_seed, layer, rows, cols, p):
    """(keep [rows][cols] bool, the f32 1 / keep as float) of dropout layer `layer` (4, 5), or (None, 1.0) without dropout."""
    if p <= 0 or layer < 4:
        return None, 1.0
    m = dropout_mask(mask_seed, layer, rows, cols, p)
    return m != 0, float(m.max())


def bn_fwd(z, bn, keep=None, drop_scale=1.0):
    """BatchNorm forward + ReLU + dropout of one layer from the device z [M][N] and the layer's parameters bn [4][N] (gamma, beta,
    moving mean, moving variance before the step) -> {name: (y, bound)} for mean, invstd, a, run_mean, run_var."""
    z = np.asarray(z, np.float64)
    M = z.shape[0]
    gamma, beta, rm, rv = (np.asarray(t, np.float64) for t in bn)
    dbl = (M + 2) * 2.0 ** -53
    mu = z.sum(axis=0) / M
    var = ((z - mu) ** 2).sum(axis=0) / M
    ez2 = (z * z).sum(axis=0) / M
    e_mean = U * np.abs(mu) + dbl * np.abs(z).sum(axis=0) / M
    e_var = (3 * M + 8) * 2.0 ** -53 * ez2
    inv = 1.0 / np.sqrt(var + BN_EPS)
    e_inv = U * inv + 0.5 * inv ** 3 * e_var + 2.0 ** -50 * inv
    gx = gamma * ((z - mu) * inv)
    y = gx + beta
    e_y = SEC * (np.abs(gamma) * inv * e_mean + np.abs(gamma) * np.abs(z - mu) * e_inv + U * (3 * np.abs(gx) + np.abs(y)))
    a = np.maximum(y, 0.0)
    e_a = e_y
    if keep is not None:
        a = np.where(keep, a * drop_scale, 0.0)
        e_a = np.where(keep, SEC * (e_y * drop_scale + U * np.abs(a)), 0.0)
    unb = var * M / (M - 1) if M > 1 else var
    r_mean = MOM * rm + ONE_MINUS_MOM * mu
    r_var = MOM * rv + ONE_MINUS_MOM * unb
    e_rm = SEC * (U * (np.abs(MOM * rm) + np.abs(ONE_MINUS_MOM * mu) + np.abs(r_mean)) + ONE_MINUS_MOM * e_mean)
    e_rv = SEC * (U * (np.abs(MOM * rv) + 2 * np.abs(ONE_MINUS_MOM * unb) + np.abs(r_var)) + ONE_MINUS_MOM * e_var * M / max(M - 1, 1))
    return {"mean": (mu, e_mean), "invstd": (inv, e_inv), "a": (a, e_a), "run_mean": (r_mean, e_rm), "run_var": (r_var, e_rv)}


def relu_mask(z, mean, invstd, bn):
    """The mask bn_grad_in recomputes, from the device z and the STORED f32 mean / invstd -> (mask bool [M][N] from the float64
    pre-activation, ambiguous bool [M][N]: within the f32 evaluation's own bound of zero)."""
    z, mean, invstd = (np.asarray(t, np.float64) for t in (z, mean, invstd))
    gamma, beta = np.asarray(bn[0], np.float64), np.asarray(bn[1], np.float64)
    gx = gamma * ((z - mean) * invstd)
    y = gx + beta
    return y > 0, np.abs(y) <= SEC * U * (3 * np.abs(gx) + np.abs(y))


def bn_bwd(go, z, mean, invstd, bn, mask, keep=None, drop_scale=1.0):
    """BatchNorm backward of one layer from the kept d loss / d a (go), the device z, the stored mean / invstd and a ReLU mask
    -> {name: (y, bound)} for dz [M][N], dgamma [N], dbeta [N]."""
    go, z, mean, invstd = (np.asarray(t, np.float64) for t in (go, z, mean, invstd))
    gamma = np.asarray(bn[0], np.float64)
    M = z.shape[0]
    dbl = (M + 2) * 2.0 ** -53
    u_drop = 0.0
    g = np.where(mask, go, 0.0)
    if keep is not None:
        g = np.where(keep, g * drop_scale, 0.0)
        u_drop = U
    xh = (z - mean) * invstd
    db = g.sum(axis=0)
    dg = (g * xh).sum(axis=0)
    e_b = SEC * (U * np.abs(db) + (u_drop + dbl) * np.abs(g).sum(axis=0))
    e_g = SEC * (U * np.abs(dg) + (2 * U + u_drop + dbl) * np.abs(g * xh).sum(axis=0))
    gi = gamma * invstd
    dz = gi * (g - (db + xh * dg) / M)
    e_dz = SEC * np.abs(gi) * (U * (4 * np.abs(g) + 6 * np.abs(db) / M + 9 * np.abs(xh * dg) / M) + (e_b + np.abs(xh) * e_g) / M)
    return {"dz": (dz, e_dz), "dgamma": (dg, e_g), "dbeta": (db, e_b)}


def bn_bwd_ratios(dev_dz, dev_dgamma, dev_dbeta, go, z, mean, invstd, bn, keep=None, drop_scale=1.0, cap=MASK_CAP):
    """Worst |dev - y| / bound of dz, dgamma and dbeta over every element, with the recomputed-mask exception of the module docstring
    -> ({"dz": r, "dgamma": r, "dbeta": r}, number of ambiguous elements).  Asserts the cap before looking at the device."""
    mask, amb = relu_mask(z, mean, invstd, bn)
    if keep is not None:
        amb = amb & keep                                     # a dropped element is 0 on either side
    n_amb = int(amb.sum())
    assert n_amb <= cap, f"{n_amb} pre-activations within rounding of zero: pick another seed"
    ref = bn_bwd(go, z, mean, invstd, bn, mask, keep, drop_scale)
    dev = {"dz": np.asarray(dev_dz, np.float64), "dgamma": np.asarray(dev_dgamma, np.float64), "dbeta": np.asarray(dev_dbeta, np.float64)}

    def col_ratios(ref_c, cols):
        return {k: ratio(dev[k][..., cols], ref_c[k][0], ref_c[k][1]) for k in dev}
    cols = np.flatnonzero(amb.any(axis=0))
    rest = np.setdiff1d(np.arange(z.shape[1]), cols)
    out = col_ratios({k: (v[0][..., rest], v[1][..., rest]) for k, v in ref.items()}, rest)
    for c in cols:                                           # every choice of the column's ambiguous elements; the best one counts
        rows = np.flatnonzero(amb[:, c])
        sl = slice(c, c + 1)
        best = None
        for bits in range(1 << len(rows)):
            m = mask[:, sl].copy()
            m[rows, 0] = [(bits >> i) & 1 for i in range(len(rows))]
            rc = bn_bwd(go[:, sl], z[:, sl], np.asarray(mean)[sl], np.asarray(invstd)[sl], np.asarray(bn)[:, sl], m,
                        None if keep is None else keep[:, sl], drop_scale)
            r = col_ratios(rc, [c])
            if best is None or max(r.values()) < max(best.values()):
                best = r
        out = {k: max(out[k], best[k]) for k in out}
    return out, n_amb


# ---- the heads --------------------------------------------------------------------------------------------------------
def heads_stage1(a5, P):
    """k_heads_loss's dot products from the device a[5] [b][512] -> {"logits": (y [b][7], bound), "v": (y [b], bound)}: 512 products
    and a bias each in f32 (a lane's 8 strided terms, then the shuffle tree), tanhf at 5 ulp behind a 1-Lipschitz tanh."""
    a = np.asarray(a5, np.float64)
    pw, pb, vw, vb = P["pi_w"], P["pi_b"], P["v_w"].reshape(512), P["v_b"].reshape(())
    lg = a @ pw + pb
    e_lg = SEC * 513 * U * (np.abs(a) @ np.abs(pw) + np.abs(pb))
    pre = a @ vw + vb
    e_pre = SEC * 513 * U * (np.abs(a) @ np.abs(vw) + np.abs(vb))
    v = np.tanh(pre)
    return {"logits": (lg, e_lg), "v": (v, SEC * (e_pre + ULP_TANH * ULP * np.abs(v)))}


def heads_stage2(logits_dev, v_dev, tpi, tv):
    """k_heads_loss's second half from the logits [b][7] and v [b] the device stored and the f32 targets -> {"loss": (y [b][2], bound),
    "dhead": (y [b][8], bound)}.  Operation by operation:
      d_o = logit_o - max (u |d_o|), e_o = expf(d_o): relative error u |d_o| + 3 ulp; se = sum e_o (six additions of positive terms);
      lse = max + logf(se): |log| 3 ulp + the relative error of se, then one addition; ls_o = logit_o - lse;
      loss_pi = - sum t_o ls_o (a product and an addition per term); softmax_o = expf(ls_o); tsum = sum t_o (six additions);
      dhead_o = (softmax_o tsum - t_o) / b: a product, a subtraction, a division;
      dv = v - t; loss_v = dv^2; dhead_7 = 2 dv (1 - v v) / b."""
    lg, v = np.asarray(logits_dev, np.float64), np.asarray(v_dev, np.float64)
    t, tv = np.asarray(tpi, np.float64), np.asarray(tv, np.float64)
    b = lg.shape[0]
    mx = lg.max(axis=1, keepdims=True)
    d = lg - mx
    e = np.exp(d)
    se = e.sum(axis=1, keepdims=True)
    rel_se = ((U * np.abs(d) + ULP_EXP * ULP) * e).sum(axis=1, keepdims=True) / se + 6 * U
    lse = mx + np.log(se)
    e_lse = ULP_LOG * ULP * np.abs(np.log(se)) + rel_se + U * np.abs(lse)
    ls = lg - lse
    e_ls = e_lse + U * np.abs(ls)
    lp = -(t * ls).sum(axis=1)
    e_lp = SEC * ((t * e_ls).sum(axis=1) + 8 * U * np.abs(t * ls).sum(axis=1))
    tsum = t.sum(axis=1, keepdims=True)
    sm = np.exp(ls)
    rel_sm = e_ls + ULP_EXP * ULP
    prod = sm * tsum
    dh = (prod - t) / b
    e_dh = SEC * ((rel_sm + 7 * U) * prod + 2 * U * np.abs(prod - t)) / b
    dv = v - tv
    lv = dv * dv
    e_lv = SEC * 3 * U * lv
    om = 1.0 - v * v
    d7 = 2.0 * dv * om / b
    e_d7 = SEC * (U * (v * v + np.abs(om)) * 2 * np.abs(dv) / b + 4 * U * np.abs(d7))
    return {"loss": (np.stack([lp, lv], axis=1), np.stack([e_lp, e_lv], axis=1)),
            "dhead": (np.concatenate([dh, d7[:, None]], axis=1), np.concatenate([e_dh, e_d7[:, None]], axis=1))}


def heads_bwd(a5, dhead_dev, P):
    """k_heads_bwd from the device a[5] and dhead [b][8] -> {"pi_w", "pi_b", "v_w", "v_b": gradients, "da": d loss / d a[5] [b][512]},
    each (y, bound): sequential f32 sums over the batch (b products), eight products for da."""
    a, dh = np.asarray(a5, np.float64), np.asarray(dhead_dev, np.float64)
    b = a.shape[0]
    pw, vw = P["pi_w"], P["v_w"].reshape(512)
    gw = a.T @ dh
    e_gw = SEC * (b + 1) * U * (np.abs(a).T @ np.abs(dh))
    gb = dh.sum(axis=0)
    e_gb = SEC * b * U * np.abs(dh).sum(axis=0)
    w8 = np.concatenate([pw, vw[:, None]], axis=1)
    da = dh @ w8.T
    e_da = SEC * 9 * U * (np.abs(dh) @ np.abs(w8).T)
    return {"pi_w": (gw[:, :7].reshape(-1), e_gw[:, :7].reshape(-1)), "v_w": (gw[:, 7], e_gw[:, 7]),
            "pi_b": (gb[:7], e_gb[:7]), "v_b": (gb[7:], e_gb[7:]), "da": (da, e_da)}


# ---- the cases of tests/test_train_layers_gpu.py (here, so that the CPU module can check their seeds) ------------------------------------
DEFAULT_SET = (1, 1, 1)
GEMM_SETS = [(1, 1, 1), (1, 1, 0), (0, 1, 0), (0, 0, 0)]          # tests/test_train_gpu.py: (train_gemm, train_fwd_dma, train_fwd_x3)
# (C, gemm set, {option: 0} switched off alone, batch); parameters net_ref.random_params(C, case_seeds()[0]), batch make_batch(b, [1])
TABLE_CASES = ([(128, gs, {}, b) for gs in GEMM_SETS for b in (2, 11, 37, 65, 128)] +
               [(256, DEFAULT_SET, {}, b) for b in (16, 32, 48)] +
               [(256, DEFAULT_SET, {sw: 0}, 32) for sw in ("train_implicit", "train_wgrad_tr", "train_gemm3_ring")] +
               [(384, DEFAULT_SET, {}, 37), (512, DEFAULT_SET, {}, 32), (512, (0, 1, 0), {}, 32)])


def case_seeds(C, b):
    return 7000 + C + b, 8000 + C + b


def case_id(case):
    C, gs, sw, b = case
    return f"C{C}-b{b}-set{''.join(map(str, gs))}" + "".join(f"-{k}0" for k in sw)


# case id -> the routes the case is in the table for, in the words of tests/train_plan_twin.decode ({"gathered": bool}, {field: {layer:
# value}}, layers 0..5 = conv1..conv4, fc1, fc2).  tests/test_train_plan_cpu.py holds the step plan (csrc/az_train_plan.h) to every entry.
def _table_routes():
    bn = lambda small: {l: "small" if l in small else "large" for l in range(6)}
    gathered = {"gathered": True, "wgrad": {1: "tr_gather", 2: "tr_gather", 3: "tr_gather"}, "dgrad": {1: "x3_gather"}, "col2im": {1: False, 2: True, 3: True}}
    fc = lambda route: {4: route, 5: route}
    out = {}
    for gs in GEMM_SETS:
        x3 = gs[0] == 1
        convs = {l: "transpose" if x3 else "f32" for l in (1, 2, 3)}
        for b, spec in (
            (2, {"bn": bn((2, 3, 4, 5))}),                        # conv1 / conv2 have 84 rows: the large-row kernels; one launch for the rest
            (11, {"bn": bn((4, 5))}),                             # conv4's (66 rows) on the large-row kernels
            (37, {"gathered": False, "wgrad": {0: "f32", **convs, **fc("transpose" if x3 else "f32")}}),      # odd: transposes + launch_gemm3, ragged tiles
            (65, {"bn": bn(())}),                                 # the FC BatchNorm on the large-row kernels
            (128, {"fwd_kernel": fc("gemm_f32_dma" if gs[1] else "gemm_f32_64"), "wgrad": {**convs, **fc("tr_act" if x3 else "f32")}}),
        ):
            out[case_id((128, gs, {}, b))] = spec
    for b, fcw in ((16, "transpose"), (32, "tr_act"), (48, "transpose")):
        out[case_id((256, DEFAULT_SET, {}, b))] = {**gathered, "wgrad": {**gathered["wgrad"], **fc(fcw)}}
    out[case_id((256, DEFAULT_SET, {"train_implicit": 0}, 32))] = {
        "gathered": False, "fwd": {1: "x3_col", 2: "x3_col", 3: "x3_col"}, "wgrad": {1: "tr_col", 2: "tr_col", 3: "tr_col", **fc("tr_act")},
        "dgrad": {1: "x3", 2: "x3", 3: "x3"}, "col2im": {1: True, 2: True, 3: True}, "im2col": {l: {"f16", "bf16"} for l in range(3)}}
    out[case_id((256, DEFAULT_SET, {"train_wgrad_tr": 0}, 32))] = {"gathered": False, "wgrad": {l: "transpose" for l in range(1, 6)}}
    out[case_id((256, DEFAULT_SET, {"train_gemm3_ring": 0}, 32))] = {        # a gathered A exists on the ring kernel only; every other x 3 GEMM on k_gemm3
        **gathered, "fwd_kernel": {1: "gemm3_ring", 2: "gemm3_ring", 3: "gemm3_ring"}, "dgrad_kernel": {1: "gemm3_ring", 2: "gemm3", 3: "gemm3", 4: "gemm3", 5: "gemm3"}}
    out[case_id((384, DEFAULT_SET, {}, 37))] = {"gathered": False, "wgrad": {l: "transpose" for l in range(1, 6)}}      # 9 C % 256 != 0
    out[case_id((512, DEFAULT_SET, {}, 32))] = {**gathered, "wgrad": {**gathered["wgrad"], **fc("tr_act")}}
    out[case_id((512, (0, 1, 0), {}, 32))] = {"gathered": False, "fwd": {l: "f32" for l in range(6)}, "wgrad": {l: "f32" for l in range(6)},
                                              "dgrad": {l: "f32" for l in range(1, 6)}}
    return out


TABLE_ROUTES = _table_routes()


# ---- the whole step, kernel by kernel -----------------------------------------------------------------------------------
def check_step(dev, p, C, boards, pis, vs, gemm_set=(1, 1, 1), mask_seed=0, dropout=0.0):
    """Every kernel of one step against its reference.  dev: {"z", "a", "mean", "invstd", "dact", "dz": lists of six arrays as read,
    "logits", "dhead", "loss": arrays, "grads": the step's gradient vector, "params_after": the parameters train_end stored}.
    -> ({kernel name: worst err / bound over every element}, {layer name: ambiguous mask elements})."""
    P = unpack64(p, C)
    off = layout(C)[0]
    g = np.asarray(dev["grads"], np.float64)
    after = np.asarray(dev["params_after"], np.float64)
    b = boards.shape[0]
    out, amb = {}, {}

    def put(name, r):
        out[name] = max(out.get(name, 0.0), r)
    for l in range(6):
        nm, N = NAMES[l], n_out(C)[l]
        a_in = boards if l == 0 else dev["a"][l - 1]
        y, bd = fwd_gemm(l, C, a_in, P, gemm_format("fwd", l, gemm_set))
        put(f"{nm} fwd gemm", ratio(dev["z"][l], y, bd))
        keep, scale = drop_of(mask_seed, l, b * ROWS_PER[l], N, dropout)
        bn = P[nm + "_bn"]
        f = bn_fwd(dev["z"][l], bn, keep, scale)
        o = off[nm + "_bn"][0]
        for k, d in (("mean", dev["mean"][l]), ("invstd", dev["invstd"][l]), ("a", dev["a"][l]),
                     ("run_mean", after[o + 2 * N:o + 3 * N]), ("run_var", after[o + 3 * N:o + 4 * N])):
            put(f"{nm} bn fwd {k}", ratio(d, *f[k]))
        r, amb[nm] = bn_bwd_ratios(dev["dz"][l], g[o:o + N], g[o + N:o + 2 * N], dev["dact"][l], dev["z"][l], dev["mean"][l],
                                   dev["invstd"][l], bn, keep, scale)
        for k, v in r.items():
            put(f"{nm} bn bwd {k}", v)
        assert np.all(g[o + 2 * N:o + 4 * N] == 0), nm                   # the moving averages have no gradient
        ob = off[nm + "_b"][0]
        assert np.all(g[ob:ob + N] == 0), f"{nm}: a bias in front of a BatchNorm has gradient exactly 0"
        ow, shp = off[nm + "_w"]
        y, bd = wgrad(l, C, a_in, dev["dz"][l], gemm_format("wgrad", l, gemm_set))
        put(f"{nm} wgrad", ratio(g[ow:ow + int(np.prod(shp))], y, bd))
        if l >= 1:
            y, bd = dgrad(l, C, dev["dz"][l], P, gemm_format("dgrad", l, gemm_set))
            put(f"{nm} dgrad", ratio(dev["dact"][l - 1], y.reshape(dev["dact"][l - 1].shape), bd.reshape(dev["dact"][l - 1].shape)))
    s1 = heads_stage1(dev["a"][5], P)
    put("heads logits", ratio(dev["logits"][:, :7], *s1["logits"]))
    put("heads v", ratio(dev["logits"][:, 7], *s1["v"]))
    s2 = heads_stage2(dev["logits"][:, :7], dev["logits"][:, 7], pis, vs)
    put("heads loss", ratio(dev["loss"], *s2["loss"]))
    put("heads dhead", ratio(dev["dhead"], *s2["dhead"]))
    hb = heads_bwd(dev["a"][5], dev["dhead"], P)
    for k in ("pi_w", "pi_b", "v_w", "v_b"):
        o, shp = off[k]
        put(f"heads d{k}", ratio(g[o:o + int(np.prod(shp))], *hb[k]))
    put("heads da", ratio(dev["dact"][5], *hb["da"]))
    return out, amb


def emulate_forward_f32(p, C, boards, mask_seed=0, dropout=0.0):
    """A plain float32 emulation of the forward (torch on the CPU) -> per layer, the number of pre-activations y = gamma xhat + beta
    that lie within the f32 evaluation's own bound of zero: the elements relu_mask would call ambiguous.  Used to choose seeds."""
    P = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in unpack64(p, C).items()}
    b = boards.shape[0]
    x = torch.from_numpy(np.asarray(boards, np.float32).reshape(b, 2, 6, 7))
    counts = {}
    for l in range(6):
        nm = NAMES[l]
        if l < 4:
            z = F.conv2d(x, P[nm + "_w"].permute(3, 2, 0, 1), P[nm + "_b"], padding=GEO[l][2])
            z = z.permute(0, 2, 3, 1).reshape(-1, C)
        else:
            z = x.reshape(b, -1) @ P[nm + "_w"] + P[nm + "_b"]
        bn = P[nm + "_bn"]
        mu = z.double().mean(dim=0)
        inv = (1.0 / torch.sqrt(z.double().var(dim=0, unbiased=False) + BN_EPS)).float()
        gx = bn[0] * ((z - mu.float()) * inv)
        y = gx + bn[1]
        near = (y.abs().double() <= SEC * U * (3 * gx.abs().double() + y.abs().double()))
        a = torch.relu(y)
        keep, scale = drop_of(mask_seed, l, z.shape[0], z.shape[1], dropout)
        if keep is not None:
            near = near & torch.from_numpy(keep)
            a = torch.where(torch.from_numpy(keep), a * np.float32(scale), torch.zeros_like(a))
        counts[nm] = int(near.sum())
        if l < 3:
            x = a.reshape(b, GEO[l][0] + 2 * GEO[l][2] - 2, GEO[l][1] + 2 * GEO[l][2] - 2, C).permute(0, 3, 1, 2)
        else:
            x = a.reshape(b, -1)                     # conv4's [b][2][3][C] flattened is fc1's input; the FC rows as they are
    return counts
