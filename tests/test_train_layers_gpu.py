"""Every kernel of one NNet::train step (csrc/az_train.hip) against its own float64 reference, element for element.

tests/test_train_gpu.py and tests/test_train_shapes_gpu.py compare a step's losses and gradients with float64 autograd END TO END, at a
bar of 1e-3 that one ReLU flip dictates.  Here the step is taken apart: the diagnostic library's az_diag_train_read copies out what the
device fed to each kernel (z, a, mean, invstd of every layer, the heads' logits / dhead / per-sample losses, and -- with
az_diag_train_keep on -- every layer's d loss / d a and dz, which otherwise share one scratch), tests/train_layers_ref.py computes that
one kernel's output from it in float64, and EVERY element must lie within a bound derived from the kernel's operand formats (that
module's docstring; tests/test_train_layers_cpu.py shows the bounds tell a wrong kernel from a right one).  The bar is
err / bound <= 1 for every kernel, case and element.

Shapes: the smallest that reach every chain of enqueue_step (train_layers_ref.TABLE_CASES, each one step with apply = False), plus
the inputs of the end-to-end tests that had to run at wide bars: dropout on the large-row kernels, the two degenerate BatchNorm
inputs, the four f16 x 3 range inputs.

Every case also asserts that losses and gradients are bit-identical with keep on and off, that the shipped library has no reader
symbol, and the reader's refusals (no such layer, rows <= 0 or > b, no step taken yet, keep while "train_fork" is 1).

Each case prints its largest err / bound per kernel class ("[layers]").

Largest err / bound seen on the MI355X, smallest .. largest over the 39 printed steps (information; the bar is 1):
    fwd gemm         0.053 .. 0.088      (f32, and f16 x 3 at K = 1152 .. 4608: the worst-case accumulation term dominates)
    wgrad            0.024 .. 0.567      (largest at b = 2, where K = rows = 2 .. 84 and the bf16 x 3 format term dominates)
    dgrad            0.002 .. 0.024
    bn fwd mean      0.960 .. 0.999      bn fwd invstd   0.932 .. 0.995      bn fwd a       0.753 .. 0.967
    bn fwd run_mean  0.825 .. 0.929      bn fwd run_var  0.782 .. 0.979
    bn bwd dz        0.498 .. 0.691      bn bwd dgamma   0.000 .. 0.788      bn bwd dbeta   0.926 .. 1.000 (below 1 before printing)
    heads logits     0.000 .. 0.001      heads v         0.000 .. 0.001      heads loss     0.078 .. 0.886
    heads dhead      0.081 .. 0.504      heads da        0.300 .. 0.553      heads dpi_w    0.024 .. 0.629
    heads dpi_b      0.004 .. 0.496      heads dv_w      0.016 .. 0.322      heads dv_b     0.000 .. 0.108
The BatchNorm statistics sit just under 1 by construction: their bound is the half ulp of the one f32 rounding behind a double sum, and
among a layer's 128 .. 1024 columns some value always rounds almost half an ulp.  Ambiguous mask elements: 0 in every table case, 1 in
two of the f16-range cases (cap 4).  The whole module took 15 s.
"""
import numpy as np
import pytest

import train_layers_ref as R
from net_ref import random_params
from test_train_gpu import make_batch, perturbed_params, set_gemms
from test_train_shapes_gpu import _identical_rows, _large_beta, _one_outlier, _zero_conv3_channel

pytestmark = pytest.mark.gpu

SWITCHES = ("train_implicit", "train_wgrad_tr", "train_gemm3_ring")


@pytest.fixture(scope="module")
def engines(engine_mod):
    """One diagnostic-library engine per width, made when a case first asks for it."""
    made = {}

    def get(C):
        if C not in made:
            made[C] = engine_mod.Engine(device=0, max_batch=256, net_channels=C, diag=True)
        return made[C]
    yield get
    for e in made.values():
        e.close()


def _options(e, gemm_set, switches, dropout):
    set_gemms(e, gemm_set)
    for sw in SWITCHES:
        e.set_option(sw, switches.get(sw, 1))
    e.set_option("train_fork", 0)
    e.set_option("train_dropout_e6", int(round(dropout * 1e6)))


def _classes(ratios):
    """{kernel name: ratio} -> the worst per kernel class (the layer names dropped), for the printed line."""
    out = {}
    for k, v in ratios.items():
        cls = k.split(" ", 1)[1] if k.split(" ", 1)[0] in R.NAMES else k
        out[cls] = max(out.get(cls, 0.0), v)
    return out


def run_case(engine_mod, e, C, p, batch, what, gemm_set=R.DEFAULT_SET, switches={}, mask_seed=0, dropout=0.0):
    """One kept step from parameters p (stored as model 1) taken apart kernel by kernel -> {kernel: worst err / bound}."""
    boards, pis, vs = batch
    b = boards.shape[0]
    try:
        _options(e, gemm_set, switches, dropout)
        e.net_set_params(1, p)
        e.train_begin(1)
        assert R.refuses(e, R.Z, 0, 1) and R.refuses(e, R.LOGITS, 0, 1), "no step taken yet"
        e.set_option("train_fork", 1)
        assert not R.set_keep(e, True), "keep while the fork is on"
        e.set_option("train_fork", 0)
        assert R.set_keep(e, True)
        (lp, lv), g = e.train_step(boards, pis, vs, mask_seed=mask_seed, apply=False, want_grads=True)
        assert np.isfinite([lp, lv]).all() and np.isfinite(g).all(), what
        for layer in (-1, 6):
            assert R.refuses(e, R.Z, layer, 1) and R.refuses(e, R.KEPT_DZ, layer, 1) and R.refuses(e, R.MEAN, layer, 1), layer
        for rows in (0, -1, b + 1):
            assert R.refuses(e, R.A, 0, rows) and R.refuses(e, R.DHEAD, 0, rows) and R.refuses(e, R.KEPT_DACT, 5, rows), rows
        assert R.refuses(e, 9, 0, 1) and R.refuses(e, -1, 0, 1)
        dev = {"grads": g}
        for name, what_id in (("z", R.Z), ("a", R.A), ("mean", R.MEAN), ("invstd", R.INVSTD), ("dact", R.KEPT_DACT), ("dz", R.KEPT_DZ)):
            dev[name] = [R.read(e, what_id, l, b, C) for l in range(6)]
        for name, what_id in (("logits", R.LOGITS), ("dhead", R.DHEAD), ("loss", R.LOSS)):
            dev[name] = R.read(e, what_id, 0, b, C)
        assert np.array_equal(R.read(e, R.Z, 2, 1, C), dev["z"][2][:R.ROWS_PER[2]])              # fewer rows: the same leading rows
        e.train_end(2)
        dev["params_after"] = e.net_get_params(2)
        # the step's losses are the per-sample losses' means (k_heads_bwd sums them in double)
        assert abs(lp - dev["loss"][:, 0].astype(np.float64).mean()) <= 2.0 ** -23 * abs(lp), what
        assert abs(lv - dev["loss"][:, 1].astype(np.float64).mean()) <= 2.0 ** -23 * abs(lv), what
        # keep off: the same bits, and nothing kept to read
        assert R.set_keep(e, False)
        e.train_begin(1)
        (lp0, lv0), g0 = e.train_step(boards, pis, vs, mask_seed=mask_seed, apply=False, want_grads=True)
        assert (lp0, lv0) == (lp, lv) and np.array_equal(g0, g), f"{what}: keep changed the step"
        assert R.refuses(e, R.KEPT_DZ, 0, 1) and R.refuses(e, R.KEPT_DACT, 0, 1)
        assert np.array_equal(R.read(e, R.Z, 5, b, C), dev["z"][5]) and np.array_equal(R.read(e, R.A, 0, b, C), dev["a"][0])
        for sym in ("az_diag_train_read", "az_diag_train_keep"):
            assert not hasattr(engine_mod._lib, sym) and hasattr(e._lib, sym), sym
        ratios, amb = R.check_step(dev, p, C, boards, pis, vs, gemm_set, mask_seed, dropout)
    finally:
        R.set_keep(e, False)
        _options(e, R.DEFAULT_SET, {}, 0.0)
    worst = max(ratios, key=ratios.get)
    print(f"[layers] {what}: worst {ratios[worst]:.3f} ({worst}); " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_classes(ratios).items())) +
          f"; ambiguous mask elements {sum(amb.values())}")
    bad = {k: v for k, v in ratios.items() if not v <= 1}
    assert not bad, (what, bad)
    assert max(amb.values()) <= R.MASK_CAP, (what, amb)
    return ratios


@pytest.mark.parametrize("case", R.TABLE_CASES, ids=R.case_id)
def test_every_kernel_meets_its_bound(engine_mod, engines, case):
    """The table of train_layers_ref.TABLE_CASES: C = 128 in all four GEMM sets at batches 2 (one-launch BatchNorm from conv3 up), 11
    (conv4's on the large-row kernels), 37 (odd: transposes + launch_gemm3, ragged tiles), 65 (the FC BatchNorm large-row), 128 (the FC
    forward on k_gemm_f32_dma); C = 256 at 16 / 32 / 48 (the gathered GEMMs, fc_tr, the FC wgrad through the transposes) and at 32 with
    each shipped switch off alone; C = 384 at 37 (9 C % 256 != 0); C = 512 at 32 in the default and the f32 set."""
    C, gemm_set, switches, b = case
    ps, bs = R.case_seeds(C, b)
    run_case(engine_mod, engines(C), C, random_params(C, ps), make_batch(b, seed=bs), R.case_id(case), gemm_set, switches)


@pytest.mark.parametrize("gemm_set", [R.DEFAULT_SET, (0, 1, 0)], ids=["default", "f32"])
def test_dropout_masks_kernel_by_kernel(engine_mod, engines, gemm_set):
    """Dropout 0.3 at C = 128, b = 65 (test_dropout_on_the_large_row_kernels_c128's inputs): the keep_thresh branches of k_colreduce<1>,
    k_bn_apply and k_bn_bwd_apply with the counter RNG's masks, the 1 / keep scale included."""
    e, b = engines(128), 65
    p = perturbed_params(e, 1, seed=3000 + b, C=128)
    run_case(engine_mod, e, 128, p, make_batch(b, seed=4000 + b), f"C=128 b=65 dropout {gemm_set}", gemm_set,
             mask_seed=0xABCDEF0123 + b, dropout=0.3)


@pytest.mark.parametrize("C", [128, 512])
def test_zero_variance_batchnorm_kernel_by_kernel(engine_mod, engines, C):
    """test_zero_variance_batchnorm's two inputs.  With two identical boards the gradients below the FC layers are 0 in exact arithmetic
    and rounding residue on the device; teacher-forced, every kernel that produces that residue is held to its own bound -- which
    answers whether the residue is a kernel's fault (see that test's docstring for the figures)."""
    e = engines(C)
    p = perturbed_params(e, 1, seed=9000 + C, C=C)
    r = run_case(engine_mod, e, C, p, _identical_rows(C), f"C={C} identical rows")
    assert max(r.values()) <= 1
    p = _zero_conv3_channel(e, C, seed=9100 + C)
    run_case(engine_mod, e, C, p, make_batch(64, seed=9200 + C), f"C={C} b=64 constant conv3 channel")


@pytest.mark.parametrize("case", ["beta_conv1", "beta_conv2", "beta_conv3", "one_outlier"])
def test_f16x3_forward_range_kernel_by_kernel(engine_mod, engines, case):
    """test_f16x3_forward_range's four inputs (activations near 1500 entering the f16 x 3 forward, C = 512, b = 64).  End to end they
    need a 5e-2 bar; teacher-forced they take the same bounds as everything else, the moving averages included.  The reference asserts
    that the scaled operands are finite in half precision."""
    e = engines(512)
    p, batch = _one_outlier(e) if case == "one_outlier" else _large_beta(e, int(case[-1]))
    run_case(engine_mod, e, 512, p, batch, f"C=512 b=64 {case}")
