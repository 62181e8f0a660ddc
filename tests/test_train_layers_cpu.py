"""The per-kernel bounds of tests/train_layers_ref.py can tell a wrong training kernel from a right one (no GPU).

Every kernel class of csrc/az_train.hip is emulated in numpy -- f32 accumulation, the bf16 and f16 hi / lo splits with three products,
the BatchNorm kernels' double sums and f32 element arithmetic, im2col / col2im by index -- and fed to the SAME reference functions and
bounds the GPU module uses.  The honest emulation must meet its bound with every element compared; each mutant (a lost cross term, a
dropped K-step, a dropped ragged row block, swapped taps, a transposed weight block, another board's rows, a mean over M - 1 rows, a
wrong mask element, a missing 1 / keep, dgamma and dbeta swapped, col2im without one tap) must exceed it.

The lost cross term is the one mutant the worst-case accumulation term can hide: on operands with random signs it is a random walk of
2^-8 (bf16) or 2^-11 (f16) of each product at most and falls under n_acc 2^-23 S once K is a few hundred.  It is shown twice: at K = 64 on random
data, and at K = 128 on operands whose low parts all have one sign (the error is then coherent, as a systematic fault's would be).
"""
import numpy as np
import pytest

import train_layers_ref as R
from net_ref import layout, random_params
from test_train_gpu import make_batch

C = 32                      # a width no kernel runs at: the reference and the emulation only need the layouts
RNG = np.random.default_rng(20240607)


@pytest.fixture(autouse=True)
def _reseed():
    """Every test draws from the same stream, whatever ran before it."""
    global RNG
    RNG = np.random.default_rng(20240607)


# ---- emulations ---------------------------------------------------------------------------------------------------------------------
def emul_gemm(a, w, fmt, s_act=64.0, drop=None):
    """[M][K] x [K][N] as the kernels compute it: f32 products and sums; or three products of the split operands, `drop` leaving one out."""
    a, w = np.asarray(a, np.float32), np.asarray(w, np.float32)
    if fmt == "f32":
        return a @ w
    if fmt == "bf16x3":
        (ah, al), (wh, wl), post = R.split_bf16(a), R.split_bf16(w), np.float32(1.0)
    else:
        (ah, al), (wh, wl) = R.split_f16(a * np.float32(s_act)), R.split_f16(w * np.float32(256.0))
        post = np.float32(1.0 / (256.0 * s_act))
    out = ah @ wh + ah @ wl
    if drop != "lo_hi":
        out = out + al @ wh
    return out * post


def im2col(l, x, taps=range(9)):
    """k_im2col by index: x [b][H][W][Cin] f32 -> [rows][9 Cin], K = tap * Cin + ci; `taps` permutes the tap each K block reads."""
    return np.concatenate([win.reshape(-1, x.shape[3]) for t in taps for ky, kx, win in R._windows(l, x) if ky * 3 + kx == t],
                          axis=1).astype(np.float32)


def col2im(l, dcol, b, Cin, skip_tap=None):
    """k_col2im: every input cell sums the taps that read it, in f32."""
    H, W, pad = R.GEO[l]
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    out = np.zeros((b, H + 2 * pad, W + 2 * pad, Cin), np.float32)
    for t in range(9):
        if t != skip_tap:
            ky, kx = divmod(t, 3)
            out[:, ky:ky + Ho, kx:kx + Wo] += dcol[:, t * Cin:(t + 1) * Cin].reshape(b, Ho, Wo, Cin)
    return out[:, pad:pad + H, pad:pad + W].reshape(b * H * W, Cin)


def conv_inputs(l, b, relu=True):
    H, W, _ = R.GEO[l]
    x = RNG.normal(size=(b, H, W, C)).astype(np.float32)
    if relu:
        x = np.maximum(x, 0)
    P = {R.NAMES[l] + "_w": RNG.uniform(-0.1, 0.1, (3, 3, C, C)).astype(np.float32).astype(np.float64),
         R.NAMES[l] + "_b": RNG.normal(0, 0.1, C).astype(np.float32).astype(np.float64)}
    return x, P


def emul_bn_fwd(z, bn, keep=None, scale=1.0, rows=None, keep_scale=True):
    """k_bn_apply: double sums, f32 mean / invstd, the element in f32 operation by operation."""
    z = np.asarray(z, np.float32)
    zs = z.astype(np.float64)[:rows]
    M = zs.shape[0]
    mu = zs.sum(axis=0) / M
    var = np.maximum((zs * zs).sum(axis=0) / M - mu * mu, 0.0)
    mean, inv = mu.astype(np.float32), (1.0 / np.sqrt(var + R.BN_EPS)).astype(np.float32)
    g, bt, rm, rv = (np.asarray(t, np.float32) for t in bn)
    a = np.maximum(g * ((z - mean) * inv) + bt, np.float32(0))
    if keep is not None:
        a = np.where(keep, a * np.float32(scale) if keep_scale else a, np.float32(0))
    mom = np.float32(0.99)
    unb = var * M / (M - 1)
    return {"mean": mean, "invstd": inv, "a": a, "run_mean": mom * rm + (np.float32(1) - mom) * mean,
            "run_var": mom * rv + (np.float32(1) - mom) * unb.astype(np.float32)}


def emul_bn_bwd(go, z, mean, inv, bn, keep=None, scale=1.0, flip=None):
    """k_bn_bwd_apply: the recomputed mask, double sums, dz in f32; `flip` = (row, column) of one mask element cut on the wrong side."""
    go, z, mean, inv = (np.asarray(t, np.float32) for t in (go, z, mean, inv))
    g_, bt = np.asarray(bn[0], np.float32), np.asarray(bn[1], np.float32)
    xh = (z - mean) * inv
    mask = g_ * xh + bt > 0
    if flip is not None:
        mask[flip] = ~mask[flip]
    g = np.where(mask, go, np.float32(0))
    if keep is not None:
        g = np.where(keep, g * np.float32(scale), np.float32(0))
    db = g.astype(np.float64).sum(axis=0).astype(np.float32)
    dg = (g.astype(np.float64) * xh).sum(axis=0).astype(np.float32)
    inv_m = np.float32(1.0) / np.float32(z.shape[0])
    return {"dz": g_ * inv * (g - (db + xh * dg) * inv_m), "dgamma": dg, "dbeta": db}


def worst(dev, ref):
    return max(R.ratio(dev[k], *ref[k]) for k in dev)


# ---- the GEMM formats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "bf16x3", "f16x3"])
@pytest.mark.parametrize("K", [64, 256, 1152])
def test_honest_gemm_meets_its_bound(fmt, K):
    a = np.maximum(RNG.normal(size=(96, K)), 0).astype(np.float32)
    w = RNG.uniform(-0.1, 0.1, (K, 128)).astype(np.float32)
    y = a.astype(np.float64) @ w.astype(np.float64)
    S = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64)
    bound = R.gemm_bound(fmt, K, S, np.abs(a).sum(axis=1, keepdims=True), np.abs(w).sum(axis=0, keepdims=True), 64.0)
    r = R.ratio(emul_gemm(a, w, fmt), y, bound)
    print(f"{fmt} K={K}: err / bound {r:.3f}")
    assert r <= 1


@pytest.mark.parametrize("fmt", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("data", ["random_k64", "coherent_k128"])
def test_lost_cross_term_fails(fmt, data):
    if data == "random_k64":
        K = 64
        a = np.maximum(RNG.normal(size=(96, K)), 0).astype(np.float32)
        w = RNG.uniform(-0.1, 0.1, (K, 128)).astype(np.float32)
    else:      # a = hi + a positive low part, w > 0: the lost lo(a) hi(w) terms all have one sign
        K = 128
        step = 2.0 ** -10 if fmt == "bf16x3" else 2.0 ** -13
        a = (1.0 + step * RNG.integers(1, 3, (96, K))).astype(np.float32)
        w = RNG.uniform(0.05, 0.1, (K, 128)).astype(np.float32)
    y = a.astype(np.float64) @ w.astype(np.float64)
    S = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64)
    bound = R.gemm_bound(fmt, K, S, np.abs(a).sum(axis=1, keepdims=True), np.abs(w).sum(axis=0, keepdims=True), 64.0)
    assert R.ratio(emul_gemm(a, w, fmt), y, bound) <= 1
    r = R.ratio(emul_gemm(a, w, fmt, drop="lo_hi"), y, bound)
    print(f"{fmt} {data}: mutant err / bound {r:.2f}")
    assert r > 1


# ---- forward conv GEMM: taps, weight blocks, rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,fmt", [(1, "f16x3"), (2, "f32"), (3, "f16x3")])
def test_forward_conv_and_its_mutants(l, fmt):
    b = 3
    x, P = conv_inputs(l, b)
    P[R.NAMES[l - 1] + "_bn"] = np.stack([np.ones(C), np.zeros(C), np.zeros(C), np.ones(C)])
    w = P[R.NAMES[l] + "_w"].reshape(9 * C, C)
    bias = P[R.NAMES[l] + "_b"].astype(np.float32)
    s = R.act_scale(np.ones(C), np.zeros(C), b * R.ROWS_PER[l - 1])
    y, bound = R.fwd_gemm(l, C, x.reshape(-1, C), P, fmt)
    honest = emul_gemm(im2col(l, x), w, fmt, s) + bias
    assert R.ratio(honest, y, bound) <= 1
    taps = list(range(9)); taps[2], taps[5] = taps[5], taps[2]
    wt = w.copy(); wt[:32, :32] = wt[:32, :32].T.copy()
    other = np.roll(x, 1, axis=0)
    mixed = im2col(l, x); mixed[:4] = im2col(l, other)[:4]               # the first rows gathered from another board
    mutants = {"two taps swapped": emul_gemm(im2col(l, x, taps), w, fmt, s) + bias,
               "a transposed weight block": emul_gemm(im2col(l, x), wt, fmt, s) + bias,
               "another board's rows": emul_gemm(mixed, w, fmt, s) + bias}
    for name, m in mutants.items():
        r = R.ratio(m, y, bound)
        print(f"conv{l + 1} {fmt} {name}: err / bound {r:.1f}")
        assert r > 1, name


# ---- wgrad: K-steps and the ragged row block ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,b,fmt", [(1, 16, "bf16x3"), (2, 5, "bf16x3"), (3, 11, "f32"), (1, 2, "bf16x3")])
def test_wgrad_and_its_mutants(l, b, fmt):
    x, _ = conv_inputs(l, b)
    col = im2col(l, x)
    M = col.shape[0]
    dz = (RNG.normal(size=(M, C)) * 1e-3).astype(np.float32)
    y, bound = R.wgrad(l, C, x.reshape(-1, C), dz, fmt)
    assert R.ratio(emul_gemm(col.T, dz, fmt).reshape(-1), y, bound) <= 1
    keep = np.ones(M, bool); keep[32:64] = False
    mutants = {"a dropped 32-row K-step": keep}
    if M % 32:
        ragged = np.ones(M, bool); ragged[M // 32 * 32:] = False
        mutants["the last ragged row block dropped"] = ragged
    for name, rows in mutants.items():
        r = R.ratio(emul_gemm(col[rows].T, dz[rows], fmt).reshape(-1), y, bound)
        print(f"conv{l + 1} wgrad M={M} {fmt} {name}: err / bound {r:.1f}")
        assert r > 1, name


def test_fc_wgrad_and_dgrad():
    a = np.maximum(RNG.normal(size=(37, 6 * C)), 0).astype(np.float32)
    dz = (RNG.normal(size=(37, 1024)) * 1e-3).astype(np.float32)
    P = {"fc1_w": RNG.uniform(-0.05, 0.05, (6 * C, 1024)).astype(np.float32).astype(np.float64)}
    for fmt in ("f32", "bf16x3"):
        y, bound = R.wgrad(4, C, a, dz, fmt)
        assert R.ratio(emul_gemm(a.T, dz, fmt).reshape(-1), y, bound) <= 1
        assert R.ratio(emul_gemm(a[:32].T, dz[:32], fmt).reshape(-1), y, bound) > 1          # 37 % 32 != 0: the ragged rows dropped
        y, bound = R.dgrad(4, C, dz, P, fmt)
        w32 = P["fc1_w"].astype(np.float32)
        assert R.ratio(emul_gemm(dz, w32.T, fmt), y, bound) <= 1
        wt = w32.copy(); wt[:32, :32] = wt[:32, :32].T.copy()
        assert R.ratio(emul_gemm(dz, wt.T, fmt), y, bound) > 1


# ---- dgrad + col2im ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,fmt", [(1, "bf16x3"), (2, "bf16x3"), (3, "f32")])
def test_dgrad_col2im_and_its_mutants(l, fmt):
    b = 3
    _, P = conv_inputs(l, b)
    H, W, pad = R.GEO[l]
    M = b * (H + 2 * pad - 2) * (W + 2 * pad - 2)
    dz = (RNG.normal(size=(M, C)) * 1e-3).astype(np.float32)
    w = P[R.NAMES[l] + "_w"].reshape(9 * C, C).astype(np.float32)
    y, bound = R.dgrad(l, C, dz, P, fmt)
    dcol = emul_gemm(dz, w.T, fmt)
    assert R.ratio(col2im(l, dcol, b, C), y, bound) <= 1
    r = R.ratio(col2im(l, dcol, b, C, skip_tap=4), y, bound)
    print(f"conv{l + 1} dgrad {fmt} col2im missing one tap: err / bound {r:.1f}")
    assert r > 1
    perm = np.arange(9 * C).reshape(9, C); perm[[2, 5]] = perm[[5, 2]]
    assert R.ratio(col2im(l, dcol[:, perm.reshape(-1)], b, C), y, bound) > 1                  # two taps swapped


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------------------------
def bn_inputs(M, N, dropout):
    z = (RNG.normal(size=(M, N)) * 0.7 + RNG.normal(size=N)).astype(np.float32)
    bn = np.stack([RNG.uniform(0.5, 1.5, N), RNG.normal(0, 0.2, N), RNG.normal(0, 0.1, N), RNG.uniform(0.5, 1.5, N)]).astype(np.float32)
    keep, scale = R.drop_of(99, 4, M, N, dropout)
    return z, bn, keep, scale


@pytest.mark.parametrize("M,dropout", [(2, 0.0), (37, 0.3), (66, 0.0), (672, 0.3)])
def test_batchnorm_forward_and_its_mutants(M, dropout):
    z, bn, keep, scale = bn_inputs(M, 128, dropout)
    ref = R.bn_fwd(z, bn, keep, scale)
    assert worst(emul_bn_fwd(z, bn, keep, scale), ref) <= 1
    if M > 2:
        m = emul_bn_fwd(z, bn, keep, scale, rows=M - 1)
        r = R.ratio(m["mean"], *ref["mean"])
        print(f"M={M} mean over M - 1 rows: err / bound {r:.0f}")
        assert r > 1 and worst(m, ref) > 1
    m = emul_bn_fwd(z, bn, keep, scale)
    i = np.unravel_index(np.argsort(m["a"], axis=None)[-m["a"].size // 4], m["a"].shape)      # an ordinary positive activation
    m["a"] = m["a"].copy(); m["a"][i] = 0
    assert R.ratio(m["a"], *ref["a"]) > 1                                                   # one ReLU mask element wrong
    if dropout:
        assert R.ratio(emul_bn_fwd(z, bn, keep, scale, keep_scale=False)["a"], *ref["a"]) > 1      # a missing 1 / keep


def test_batchnorm_forward_with_zero_variance():
    z, bn, _, _ = bn_inputs(2, 128, 0.0)
    z[1] = z[0]
    assert worst(emul_bn_fwd(z, bn), R.bn_fwd(z, bn)) <= 1


@pytest.mark.parametrize("M,dropout", [(2, 0.0), (37, 0.3), (66, 0.0), (672, 0.3)])
def test_batchnorm_backward_and_its_mutants(M, dropout):
    z, bn, keep, scale = bn_inputs(M, 128, dropout)
    f = emul_bn_fwd(z, bn, keep, scale)
    go = (RNG.normal(size=z.shape) * 1e-3).astype(np.float32)
    args = (go, z, f["mean"], f["invstd"], bn, keep, scale)
    dev = emul_bn_bwd(*args)
    r, n_amb = R.bn_bwd_ratios(dev["dz"], dev["dgamma"], dev["dbeta"], *args)
    assert max(r.values()) <= 1 and n_amb == 0, r
    bad = lambda d: max(R.bn_bwd_ratios(d["dz"], d["dgamma"], d["dbeta"], *args)[0].values())
    assert bad({"dz": dev["dz"], "dgamma": dev["dbeta"], "dbeta": dev["dgamma"]}) > 1           # dgamma and dbeta swapped
    live = np.abs(go) * (keep if keep is not None else 1)
    i = np.unravel_index(np.argsort(live, axis=None)[-live.size // 4], live.shape)
    assert bad(emul_bn_bwd(*args, flip=i)) > 1                                                  # one ReLU mask element wrong
    if dropout:
        assert bad(emul_bn_bwd(go, z, f["mean"], f["invstd"], bn, keep, 1.0)) > 1               # a missing 1 / keep


def test_recomputed_mask_exception_is_confined_to_the_ambiguous_elements():
    """An element within rounding of zero may be cut on either side (both pass); the cap is asserted before the device is looked at."""
    z, bn, _, _ = bn_inputs(37, 128, 0.0)
    f = emul_bn_fwd(z, bn)
    go = (RNG.normal(size=z.shape) * 1e-3).astype(np.float32)
    bn64 = bn.astype(np.float64)
    xh = (z[5, 9].astype(np.float64) - f["mean"][9]) * f["invstd"][9]
    bn64[1, 9] = -bn64[0, 9] * xh                                    # beta that puts element (5, 9)'s pre-activation at zero
    bn = bn64.astype(np.float32)
    args = (go, z, f["mean"], f["invstd"], bn)
    assert R.relu_mask(z, f["mean"], f["invstd"], bn)[1].sum() == 1
    for flip in (None, (5, 9)):
        dev = emul_bn_bwd(*args, flip=flip)
        r, n_amb = R.bn_bwd_ratios(dev["dz"], dev["dgamma"], dev["dbeta"], *args)
        assert n_amb == 1 and max(r.values()) <= 1, (flip, r)
    dev = emul_bn_bwd(*args, flip=(6, 9))                            # its neighbour is not excused
    assert max(R.bn_bwd_ratios(dev["dz"], dev["dgamma"], dev["dbeta"], *args)[0].values()) > 1
    with pytest.raises(AssertionError):
        R.bn_bwd_ratios(dev["dz"], dev["dgamma"], dev["dbeta"], *args, cap=0)


# ---- heads ---------------------------------------------------------------------------------------------------------------------------------------
def emul_heads(a, P, pis, vs):
    """k_heads_loss + k_heads_bwd in f32 -> (logits8 [b][8], dhead [b][8], loss [b][2], {gradient name: array}, da [b][512])."""
    b = a.shape[0]
    pw, pb, vw, vb = (P[k].astype(np.float32) for k in ("pi_w", "pi_b", "v_w", "v_b"))
    lg = a @ pw + pb
    v = np.tanh((a @ vw.reshape(512) + vb).astype(np.float32)).astype(np.float32)
    mx = lg.max(axis=1, keepdims=True)
    ls = lg - (mx + np.log(np.exp(lg - mx).sum(axis=1, keepdims=True)))
    dh = np.concatenate([(np.exp(ls) * pis.sum(axis=1, keepdims=True) - pis) / np.float32(b),
                         (np.float32(2) * (v - vs) * (np.float32(1) - v * v) / np.float32(b))[:, None]], axis=1).astype(np.float32)
    loss = np.stack([-(pis * ls).sum(axis=1), (v - vs) ** 2], axis=1).astype(np.float32)
    w8 = np.concatenate([pw, vw.reshape(512, 1)], axis=1)
    gw = a.T @ dh
    grads = {"pi_w": gw[:, :7].reshape(-1), "v_w": gw[:, 7], "pi_b": dh.sum(axis=0)[:7], "v_b": dh.sum(axis=0)[7:]}
    return np.concatenate([lg, v[:, None]], axis=1), dh, loss, grads, dh @ w8.T


def test_heads_and_their_mutants():
    b = 37
    a = np.maximum(RNG.normal(size=(b, 512)), 0).astype(np.float32)
    P = {k: v for k, v in R.unpack64(random_params(128, 3), 128).items() if k.startswith(("pi", "v"))}
    _, pis, vs = make_batch(b, seed=4)
    lg8, dh, loss, grads, da = emul_heads(a, P, pis, vs)
    lg, v = lg8[:, :7], lg8[:, 7]
    s1 = R.heads_stage1(a, P)
    assert R.ratio(lg, *s1["logits"]) <= 1 and R.ratio(v, *s1["v"]) <= 1
    assert R.ratio(lg[:, ::-1], *s1["logits"]) > 1                                              # the moves in the wrong order
    s2 = R.heads_stage2(lg, v, pis, vs)
    assert R.ratio(loss, *s2["loss"]) <= 1 and R.ratio(dh, *s2["dhead"]) <= 1
    assert R.ratio(dh * np.float32(b) / np.float32(b + 1), *s2["dhead"]) > 1                    # divided by the wrong batch
    hb = R.heads_bwd(a, dh, P)
    assert R.ratio(da, *hb["da"]) <= 1 and all(R.ratio(grads[k], *hb[k]) <= 1 for k in grads)
    assert R.ratio((a[:32].T @ dh[:32])[:, :7].reshape(-1), *hb["pi_w"]) > 1                    # the batch's last five rows dropped


# ---- the whole step ------------------------------------------------------------------------------------------------------------------------------
def emulate_step(p, Cw, boards, pis, vs, gemm_set, mask_seed=0, dropout=0.0):
    """One step as enqueue_step chains the emulated kernels, every intermediate kept -> the `dev` dictionary check_step takes."""
    P = {k: v.astype(np.float32) for k, v in R.unpack64(p, Cw).items()}
    off = layout(Cw)[0]
    b = boards.shape[0]
    dev = {k: [None] * 6 for k in ("z", "a", "mean", "invstd", "dact", "dz")}
    g, after = np.zeros(p.size, np.float32), np.array(p, np.float32)
    x = np.ascontiguousarray(np.asarray(boards, np.float32).transpose(0, 2, 3, 1))
    cols, drops = [], []
    for l in range(6):
        nm, N = R.NAMES[l], R.n_out(Cw)[l]
        col = im2col(l, x) if l < 4 else x.reshape(b, -1)
        s = 64.0
        if 1 <= l <= 3:
            s = R.act_scale(P[R.NAMES[l - 1] + "_bn"][0], P[R.NAMES[l - 1] + "_bn"][1], b * R.ROWS_PER[l - 1])
        z = emul_gemm(col, P[nm + "_w"].reshape(-1, N), R.gemm_format("fwd", l, gemm_set), s) + P[nm + "_b"]
        keep, scale = R.drop_of(mask_seed, l, z.shape[0], N, dropout)
        f = emul_bn_fwd(z, P[nm + "_bn"], keep, scale)
        dev["z"][l], dev["a"][l], dev["mean"][l], dev["invstd"][l] = z, f["a"], f["mean"], f["invstd"]
        o = off[nm + "_bn"][0]
        after[o + 2 * N:o + 3 * N], after[o + 3 * N:o + 4 * N] = f["run_mean"], f["run_var"]
        cols.append(col); drops.append((keep, scale))
        if l < 3:
            H, W, pad = R.GEO[l]
            x = f["a"].reshape(b, H + 2 * pad - 2, W + 2 * pad - 2, Cw)
        else:
            x = f["a"]
    lg8, dh, loss, hg, dact = emul_heads(dev["a"][5], P, np.asarray(pis, np.float32), np.asarray(vs, np.float32))
    dev["logits"], dev["dhead"], dev["loss"] = lg8, dh, loss
    for k, v in hg.items():
        g[off[k][0]:off[k][0] + v.size] = v
    for l in range(5, -1, -1):
        nm, N = R.NAMES[l], R.n_out(Cw)[l]
        dact = dact.reshape(dev["z"][l].shape)
        dev["dact"][l] = dact
        bw = emul_bn_bwd(dact, dev["z"][l], dev["mean"][l], dev["invstd"][l], P[nm + "_bn"], *drops[l])
        dev["dz"][l] = bw["dz"]
        o = off[nm + "_bn"][0]
        g[o:o + N], g[o + N:o + 2 * N] = bw["dgamma"], bw["dbeta"]
        ow, shp = off[nm + "_w"]
        g[ow:ow + int(np.prod(shp))] = emul_gemm(cols[l].T, bw["dz"], R.gemm_format("wgrad", l, gemm_set)).reshape(-1)
        if l >= 1:
            dcol = emul_gemm(bw["dz"], P[nm + "_w"].reshape(-1, N).T, R.gemm_format("dgrad", l, gemm_set))
            dact = col2im(l, dcol, b, Cw) if l < 4 else dcol
    dev["grads"], dev["params_after"] = g, after
    return dev


@pytest.mark.parametrize("b,gemm_set,dropout", [(11, (1, 1, 1), 0.0), (5, (0, 1, 0), 0.3)])
def test_an_emulated_step_passes_kernel_by_kernel(b, gemm_set, dropout):
    """check_step itself (offsets, layouts, the chain of inputs) on a whole emulated step at C = 128; and a step with one wrong kernel
    fails in that kernel's line only."""
    p = random_params(128, 7)
    boards, pis, vs = make_batch(b, seed=8)
    dev = emulate_step(p, 128, boards, pis, vs, gemm_set, mask_seed=5, dropout=dropout)
    ratios, amb = R.check_step(dev, p, 128, boards, pis, vs, gemm_set, 5, dropout)
    assert max(ratios.values()) <= 1 and max(amb.values()) == 0, {k: v for k, v in ratios.items() if v > 1}
    assert len(ratios) == 6 * 10 + 5 + 9                       # six layers (conv1 has no dgrad) and the heads
    dev["dact"][2] = dev["dact"][2].copy(); dev["dact"][2][7] = dev["dact"][2][8]               # one row of conv4's dgrad from its neighbour
    ratios, _ = R.check_step(dev, p, 128, boards, pis, vs, gemm_set, 5, dropout)
    assert {k for k, v in ratios.items() if v > 1} == {"conv4 dgrad", "conv3 bn bwd dz", "conv3 bn bwd dgamma", "conv3 bn bwd dbeta"}


# ---- the reader's wrapper and the cases' seeds ---------------------------------------------------------------------------------------------------
class _NoLibrary:
    """An engine whose library must not be reached: read() has to refuse a bad shape before it touches it."""
    _h = None

    @property
    def _lib(self):
        raise AssertionError("the library was reached")


@pytest.mark.parametrize("what,layer,rows,width", [(9, 0, 2, 128), (-1, 0, 2, 128), (R.Z, 6, 2, 128), (R.Z, -1, 2, 128), (R.A, 0, 0, 128),
                                                   (R.A, 0, -3, 128), (R.KEPT_DZ, 0, 257, 128), (R.MEAN, 7, 2, 128), (R.Z, 0, 2, 100),
                                                   (R.Z, 0, 2.5, 128)])
def test_reader_wrapper_rejects_bad_shapes_without_a_library(what, layer, rows, width):
    with pytest.raises(ValueError):
        R.read(_NoLibrary(), what, layer, rows, width)


def test_reader_shapes():
    assert R.read_shape(R.Z, 2, 5, 256) == (100, 256) and R.read_shape(R.A, 4, 5, 256) == (5, 1024)
    assert R.read_shape(R.MEAN, 5, 5, 128) == (512,) and R.read_shape(R.LOGITS, 99, 5, 128) == (5, 8)
    assert R.read_shape(R.LOSS, 0, 7, 128) == (7, 2) and R.read_shape(R.KEPT_DACT, 3, 2, 384) == (12, 384)


def test_gemm_formats_follow_enqueue_step():
    assert [R.gemm_format("fwd", l, (1, 1, 1)) for l in range(6)] == ["f32", "f16x3", "f16x3", "f16x3", "f32", "f32"]
    assert all(R.gemm_format("fwd", l, gs) == "f32" for l in range(6) for gs in ((1, 1, 0), (0, 1, 0), (0, 0, 0), (0, 1, 1)))
    assert [R.gemm_format("wgrad", l, (1, 1, 0)) for l in range(6)] == ["f32"] + ["bf16x3"] * 5
    assert all(R.gemm_format(k, l, (0, 1, 0)) == "f32" for l in range(6) for k in ("wgrad", "dgrad"))


@pytest.mark.parametrize("C_,b", sorted({(c[0], c[3]) for c in R.TABLE_CASES}))
def test_case_seeds_stay_within_the_mask_cap(C_, b):
    """A float32 emulation of the forward at every (width, batch) of the GPU module's table, from the same seeds: at most MASK_CAP
    pre-activations per layer lie within rounding of zero (the GPU module asserts the same from the device's z before it compares)."""
    ps, bs = R.case_seeds(C_, b)
    boards, _, _ = make_batch(b, seed=bs)
    counts = R.emulate_forward_f32(random_params(C_, ps), C_, boards)
    print(C_, b, counts)
    assert max(counts.values()) <= R.MASK_CAP, counts
