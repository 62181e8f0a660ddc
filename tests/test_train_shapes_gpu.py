"""NNet::train (csrc/az_train.hip) against float64 autograd over the whole accepted range: every batch in [2, 256] and every width
C % 128 == 0 reaches a kernel chain of its own, chosen by the step plan (csrc/az_train_plan.h) from row thresholds and divisibility rules
(BN_SMALL_ROWS, k_wgrad3_tr's 32-row steps, the gathered ImplicitA GEMMs at C % 256 == 0 and b % 16 == 0, k_gemm_f32_dma at >= 128 rows,
the split-K plans).  The batches below are picked to cross those thresholds; each states the routes it is here for as data (SWEEP_512,
SWEEP_512_F32, OTHER_WIDTHS, NEW_ROUTES), and tests/test_train_plan_cpu.py holds the plan to every entry and checks that every route the
plan can choose is reached by some case that runs on the GPU.  The bars are
test_gradients_match_autograd's (tests/test_train_gpu.py check_step): losses to 1e-5 relative, every gradient tensor to 1e-3 relative L2,
pre-BN biases exactly 0, moving averages to 1e-6 / 1e-5.  check_step prints the worst per-tensor error of every case ("[worst]").
"""
import numpy as np
import pytest

from net_ref import layout
from test_train_gpu import GEMM_SET_IDS, GEMM_SETS, check_step, make_batch, mix64, perturbed_params, set_gemms
from train_ref import step_reference

pytestmark = pytest.mark.gpu


def _engine(engine_mod, C):
    e = engine_mod.Engine(device=0, max_batch=1024, net_channels=C)
    e.set_option("train_dropout_e6", 0)
    return e


@pytest.fixture(scope="module")
def e512(engine_mod):
    e = _engine(engine_mod, 512)
    yield e
    e.close()


@pytest.fixture(scope="module", params=GEMM_SETS, ids=GEMM_SET_IDS)
def e128(engine_mod, request):
    e = _engine(engine_mod, 128)
    set_gemms(e, request.param)
    yield e
    e.close()


def _restore(e):
    """The engine-wide options back to the defaults between tests (a fixture engine is shared by the module)."""
    for key, val in (("train_gemm", 1), ("train_fwd_dma", 1), ("train_fwd_x3", 1), ("train_implicit", 1), ("train_wgrad_tr", 1),
                     ("train_gemm3_ring", 1), ("train_fork", 0), ("train_graph", 1), ("train_dropout_e6", 0), ("train_epochs", 10),
                     ("train_batch", 64), ("train_seed", 0)):
        e.set_option(key, val)


# ---- the batch sweep at the shipped width ------------------------------------------------------------------------------------------

# batch -> the routes it is here for, in the words of tests/train_plan_twin.decode: {"gathered": bool} and {field: {layer: value}} with
# layers 0..5 = conv1..conv4, fc1, fc2.  tests/test_train_plan_cpu.py holds the step plan (csrc/az_train_plan.h) to every entry.
_TRANSPOSES = {l: "transpose" for l in range(1, 6)}
_GATHERED = {"gathered": True, "wgrad": {1: "tr_gather", 2: "tr_gather", 3: "tr_gather"}, "dgrad": {1: "x3_gather"}, "col2im": {1: False, 2: True, 3: True}}
_FC_DMA = {4: "gemm_f32_dma", 5: "gemm_f32_dma"}
_FC_F32_64 = {4: "gemm_f32_64", 5: "gemm_f32_64"}

SWEEP_512 = {
    # smallest batch: conv3 (40 rows) and conv4 (12) BatchNorm on k_bn_fwd_small / k_bn_bwd_small, FC on the one-launch kernels
    2: {"gathered": False, "bn": {0: "large", 1: "large", 2: "small", 3: "small", 4: "small", 5: "small"}, "wgrad": _TRANSPOSES},
    # largest batch whose conv3 BatchNorm (60 rows) is on the one-launch kernels
    3: {"bn": {1: "large", 2: "small"}},
    # b % 8: conv3's wgrad on k_wgrad3_tr from the stored operands (160 rows), conv2 / conv4 through the transposes
    8: {"gathered": False, "wgrad": {1: "transpose", 2: "tr_col", 3: "transpose"}, "im2col": {0: {"f16", "f32"}, 1: {"f16", "bf16"}, 2: {"f16", "f32"}}},
    # largest batch whose conv4 BatchNorm (60 rows) is on the one-launch kernels
    10: {"bn": {2: "large", 3: "small"}},
    # conv4 BatchNorm on k_colreduce / k_bn_apply (66 rows); odd: no k_wgrad3_tr anywhere
    11: {"bn": {3: "large", 4: "small"}, "wgrad": _TRANSPOSES},
    # smallest gathered batch (ImplicitA forward / wgrad, conv2 dgrad without col2im), FC wgrad not yet on k_wgrad3_tr
    16: {**_GATHERED, "wgrad": {**_GATHERED["wgrad"], 4: "transpose", 5: "transpose"}, "im2col": {0: None, 1: None, 2: None}},
    # b % 8 but not % 16: k_wgrad3_tr on conv3 only (480 rows), transposes on conv2 / conv4, no gathered GEMMs
    24: {"gathered": False, "wgrad": {1: "transpose", 2: "tr_col", 3: "transpose", 4: "transpose", 5: "transpose"}},
    # odd: every wgrad through k_transpose_split + launch_gemm3; the ring's waste rule at 1554 rows keeps conv2's forward and dgrad on k_gemm3
    37: {"gathered": False, "wgrad": _TRANSPOSES, "fwd_kernel": {1: "gemm3", 2: "gemm3_ring"}, "dgrad_kernel": {1: "gemm3", 2: "gemm3_ring"}},
    # the bench shape: gathered GEMMs, FC wgrad on k_wgrad3_tr, FC BatchNorm at BN_SMALL_ROWS exactly
    64: {**_GATHERED, "wgrad": {**_GATHERED["wgrad"], 4: "tr_act", 5: "tr_act"}, "bn": {3: "large", 4: "small", 5: "small"}, "fwd_kernel": _FC_F32_64},
    # FC BatchNorm on the large-row kernels (k_colreduce, k_bn_apply, k_bn_bwd_apply); odd: no gathered GEMMs
    65: {"gathered": False, "bn": {4: "large", 5: "large"}, "wgrad": _TRANSPOSES},
    # gathered + FC wgrad on k_wgrad3_tr, FC BatchNorm on the large-row kernels, 4032 / 1920 / 576 rows in the split-K plans
    96: {**_GATHERED, "wgrad": {**_GATHERED["wgrad"], 4: "tr_act", 5: "tr_act"}, "bn": {4: "large", 5: "large"}},
    # FC forward on k_gemm_f32_dma (>= 128 rows), gathered, FC wgrad on k_wgrad3_tr
    128: {**_GATHERED, "wgrad": {**_GATHERED["wgrad"], 4: "tr_act", 5: "tr_act"}, "fwd_kernel": _FC_DMA},
    # b % 8 only: k_wgrad3_tr on conv3, transposes elsewhere, FC on k_gemm_f32_dma without k_wgrad3_tr (200 % 32 != 0)
    200: {"gathered": False, "wgrad": {1: "transpose", 2: "tr_col", 3: "transpose", 4: "transpose", 5: "transpose"}, "fwd_kernel": _FC_DMA},
    # the largest batch (TRAIN_MAX_BATCH): 10752 rows in conv1 / conv2, every split-K plan at its maximum M
    256: {**_GATHERED, "wgrad": {**_GATHERED["wgrad"], 4: "tr_act", 5: "tr_act"}, "fwd_kernel": _FC_DMA},
}

# the same thresholds with every GEMM on the f32 matrix cores ("train_gemm" 0)
_ALL_F32 = {"gathered": False, "fwd": {l: "f32" for l in range(6)}, "wgrad": {l: "f32" for l in range(6)}, "dgrad": {l: "f32" for l in range(1, 6)}}
SWEEP_512_F32 = {
    2: {**_ALL_F32, "bn": {0: "large", 1: "large", 2: "small", 3: "small", 4: "small", 5: "small"}},
    11: {**_ALL_F32, "bn": {3: "large", 4: "small"}},
    24: {**_ALL_F32, "fwd_kernel": {1: "gemm_f32_dma", 2: "gemm_f32_dma", 3: "gemm_f32_dma", **_FC_F32_64}},
    65: {**_ALL_F32, "bn": {4: "large", 5: "large"}, "fwd_kernel": _FC_F32_64},
    128: {**_ALL_F32, "fwd_kernel": _FC_DMA},
    256: {**_ALL_F32, "fwd_kernel": _FC_DMA},
}


# batch -> (parameter seed, batch seed); the rest use (1000 + b, 2000 + b).  A ReLU mask flip -- a pre-activation within rounding of
# zero, cut on one side only -- moves every gradient tensor by 2e-4 .. 1e-2 at this width, at ANY batch (measured on the MI355X with
# (1000 + b, 2000 + b): b = 16 2.5e-3, 96 2.5e-3, 200 1.2e-2, 256 1.3e-3 in the f32 set; plain float32 PyTorch on the CPU, same inputs:
# 1.7e-3 at b = 200).  These seeds have none in the sets that run them; 200 and 256 are the best of six tried (1.7e-4 / 1.7e-4 and 1.3e-4
# in the f32 set: not flip-free, five times under the bar).
SEEDS_512 = {16: (8935, 9935), 64: (8983, 9983), 96: (16934, 17934), 200: (48714, 49714), 256: (48770, 49770)}


def _sweep_inputs(e, b):
    ps, bs = SEEDS_512.get(b, (1000 + b, 2000 + b))
    return perturbed_params(e, 1, seed=ps, C=512), make_batch(b, seed=bs)


@pytest.mark.parametrize("b", SWEEP_512)
def test_batch_sweep_default_set_at_c512(e512, b):
    """Default GEMM set (f16 x 3 forward, bf16 x 3 backward) at C = 512, dropout off, every threshold of enqueue_step."""
    _restore(e512)
    p, (boards, pis, vs) = _sweep_inputs(e512, b)
    check_step(e512, p, 512, boards, pis, vs, f"C=512 b={b} default")


@pytest.mark.parametrize("b", SWEEP_512_F32)
def test_batch_sweep_f32_set_at_c512(e512, b):
    """Every GEMM on the f32 matrix cores ("train_gemm" 0) over the same thresholds: the small / large BatchNorm kernels (2, 11, 65),
    the f32 forward on k_gemm_f32 (< 128 rows: the FC layers up to b = 127) and on k_gemm_f32_dma (128, 256), split-K plans."""
    _restore(e512)
    e512.set_option("train_gemm", 0)
    try:
        p, (boards, pis, vs) = _sweep_inputs(e512, b)
        check_step(e512, p, 512, boards, pis, vs, f"C=512 b={b} f32")
    finally:
        _restore(e512)


# ---- dropout on the large-row BatchNorm kernels ---------------------------------------------------------------------------------------

def _dropout_case(e, C, b, what):
    e.set_option("train_dropout_e6", 300000)
    p = perturbed_params(e, 1, seed=3000 + b, C=C)
    boards, pis, vs = make_batch(b, seed=4000 + b)
    seed = 0xABCDEF0123 + b
    (lp, lv), g, _ = check_step(e, p, C, boards, pis, vs, what, mask_seed=seed, dropout=0.3)
    # the same step again is bit-identical (fixed-order reductions, no atomics)
    e.train_begin(1)
    (lp2, lv2), g2 = e.train_step(boards, pis, vs, mask_seed=seed, apply=False, want_grads=True)
    assert (lp2, lv2) == (lp, lv) and np.array_equal(g2, g), what


DROPOUT_C128 = [65, 128, 256]


@pytest.mark.parametrize("b", DROPOUT_C128)
def test_dropout_on_the_large_row_kernels_c128(e128, b):
    """Dropout 0.3 with b > BN_SMALL_ROWS: the keep_thresh branches of k_colreduce<1>, k_bn_apply and k_bn_bwd_apply (every other
    dropout test runs the FC BatchNorm on the one-launch kernels).  The reference applies the counter RNG's masks explicitly."""
    try:
        _dropout_case(e128, 128, b, f"C=128 b={b} dropout")
    finally:
        e128.set_option("train_dropout_e6", 0)


def test_dropout_on_the_large_row_kernels_c512(e512):
    """The same at the shipped width and the largest batch, default set."""
    _restore(e512)
    try:
        _dropout_case(e512, 512, 256, "C=512 b=256 dropout")
    finally:
        _restore(e512)


# ---- other widths ------------------------------------------------------------------------------------------------------------------

OTHER_WIDTHS = {
    # gathered GEMMs at the smallest width that has them (C % 256 == 0), smallest gathered batch
    (256, 16): {**_GATHERED, "wgrad": {**_GATHERED["wgrad"], 4: "transpose", 5: "transpose"}},
    # gathered, FC wgrad through the transposes (48 % 32 != 0)
    (256, 48): {**_GATHERED, "wgrad": {**_GATHERED["wgrad"], 4: "transpose", 5: "transpose"}},
    # gathered + FC wgrad on k_wgrad3_tr
    (256, 64): {**_GATHERED, "wgrad": {**_GATHERED["wgrad"], 4: "tr_act", 5: "tr_act"}},
    # 9 C % 256 != 0: no k_wgrad3_tr on the convs, no gathered GEMMs; odd batch
    (384, 37): {"gathered": False, "wgrad": _TRANSPOSES},
    # the same at the default batch (FC wgrad on k_wgrad3_tr, K = 6 C = 2304)
    (384, 64): {"gathered": False, "wgrad": {1: "transpose", 2: "transpose", 3: "transpose", 4: "tr_act", 5: "tr_act"}},
}


@pytest.mark.parametrize("C,b", OTHER_WIDTHS)
def test_other_widths(engine_mod, C, b):
    """Training at C = 256 and 384 (inference is tested at both), default set."""
    e = _engine(engine_mod, C)
    try:
        p = perturbed_params(e, 1, seed=5000 + b, C=C)
        boards, pis, vs = make_batch(b, seed=6000 + b)
        check_step(e, p, C, boards, pis, vs, f"C={C} b={b}")
    finally:
        e.close()


# ---- routes no other GPU case reaches ------------------------------------------------------------------------------------------------

# (C, batch, {option: value}, routes): the smallest case for each per-layer route that the step plan can choose and no other case of this
# module, of tests/test_train_layers_gpu.py or of tests/test_train_gpu.py takes (tests/test_train_plan_cpu.py
# test_every_reachable_route_runs_on_the_gpu lists what would be missing without them)
NEW_ROUTES = [
    # f32 forward with k_wgrad3_tr on the convs: k_im2col writes the f32 matrix and the bf16 pairs, no half pairs (16: the smallest batch
    # at which conv2, conv3 and conv4 all have their rows in 32s)
    (256, 16, {"train_fwd_x3": 0}, {"gathered": False, "fwd": {1: "f32", 2: "f32", 3: "f32"}, "wgrad": {1: "tr_col", 2: "tr_col", 3: "tr_col"},
                                    "im2col": {0: {"f32", "bf16"}, 1: {"f32", "bf16"}, 2: {"f32", "bf16"}}}),
    # conv3's register-staged f32 forward in 128 x 128 tiles: 64 of them need 20 b > 31 x 128 rows at two column tiles
    (256, 199, {"train_gemm": 0, "train_fwd_dma": 0}, {"fwd_kernel": {1: "gemm_f32_128", 2: "gemm_f32_128", 3: "gemm_f32_64"}}),
]


@pytest.mark.parametrize("C,b,switches", [c[:3] for c in NEW_ROUTES], ids=[f"{c[0]}-{c[1]}-" + "-".join(f"{k}{v}" for k, v in c[2].items()) for c in NEW_ROUTES])
def test_routes_no_other_case_reaches(engine_mod, C, b, switches):
    e = _engine(engine_mod, C)
    try:
        for key, val in switches.items():
            e.set_option(key, val)
        p = perturbed_params(e, 1, seed=5500 + b, C=C)
        boards, pis, vs = make_batch(b, seed=6500 + b)
        check_step(e, p, C, boards, pis, vs, f"C={C} b={b} {switches}")
    finally:
        e.close()


# ---- the shipped switches -------------------------------------------------------------------------------------------------------------

SHIPPED_SWITCHES = ["train_implicit", "train_wgrad_tr", "train_gemm3_ring"]
SWITCH_BATCHES = [64, 128]


@pytest.mark.parametrize("b", SWITCH_BATCHES)
@pytest.mark.parametrize("switch", SHIPPED_SWITCHES)
def test_shipped_switches_off_at_c512(e512, switch, b):
    """Each shipped option turned off alone at C = 512: the im2col + col2im conv GEMMs instead of the gathered ones, wgrad through the
    transposes instead of k_wgrad3_tr, every x3 GEMM on k_gemm3 instead of the ring."""
    _restore(e512)
    e512.set_option(switch, 0)
    try:
        p, (boards, pis, vs) = _sweep_inputs(e512, b)
        check_step(e512, p, 512, boards, pis, vs, f"C=512 b={b} {switch}=0")
    finally:
        _restore(e512)


@pytest.mark.parametrize("b", SWITCH_BATCHES)
def test_fork_is_bit_identical_at_c512(e512, b):
    """"train_fork" 1 (the wgrad chains on a second stream branch, here around the gathered wgrad: events ev_dz / ev_tr) gives the
    same bits as 0: single steps with dropout, and a short az_net_train with the captured graph and with direct launches."""
    _restore(e512)
    try:
        e512.set_option("train_dropout_e6", 300000)
        p = perturbed_params(e512, 1, seed=1000 + b, C=512)
        boards, pis, vs = make_batch(b, seed=2000 + b)
        out = []
        for fork in (0, 1):
            e512.set_option("train_fork", fork)
            e512.train_begin(1)
            out.append(e512.train_step(boards, pis, vs, mask_seed=99, apply=False, want_grads=True))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
        e512.train_end(3)                         # az_net_train is refused while a step session is open; id 3 is overwritten below
        n = 3 * b
        tb, tp, tv = make_batch(n, seed=7000 + b)
        for key, val in (("train_epochs", 1), ("train_batch", b), ("train_seed", 5)):
            e512.set_option(key, val)
        got = {}
        for graph in (1, 0):
            for fork in (0, 1):
                e512.set_option("train_graph", graph)
                e512.set_option("train_fork", fork)
                hist = e512.train(1, 3, tb, tp, tv)
                got[graph, fork] = (hist, e512.net_get_params(3))
        for graph in (1, 0):
            assert got[graph, 0][0] == got[graph, 1][0], graph
            assert np.array_equal(got[graph, 0][1], got[graph, 1][1]), graph
        assert np.array_equal(got[1, 0][1], got[0, 0][1])
    finally:
        _restore(e512)


# ---- degenerate BatchNorm ------------------------------------------------------------------------------------------------------------

def _identical_rows(C):
    boards, pis, vs = make_batch(2, seed=8000 + C)
    boards[1] = boards[0]        # two identical boards: every FC column has variance exactly 0 (the targets differ, so dz does not vanish)
    return boards, pis, vs


def _zero_conv3_channel(e, C, seed):
    p = perturbed_params(e, 1, seed=seed, C=C)
    o, shp = layout(C)[0]["conv3_w"]
    w = p[o:o + int(np.prod(shp))].reshape(shp)              # view: [3][3][C][C], output channel last
    w[..., 7] = 0.0                                           # conv3 channel 7 is its bias at every row: variance exactly 0
    e.net_set_params(1, p)
    return p


@pytest.mark.parametrize("C", [128, 512])
def test_zero_variance_batchnorm(engine_mod, C):
    """BatchNorm with a variance of exactly 0 -- xhat = 0 / sqrt(eps), the output beta, dgamma = 0 -- in the FC layers (a batch of
    two identical boards with different targets) and in one conv3 channel (all its weights 0).  The reference uses the same eps = 1e-3.
    With two identical boards the dz of every BatchNorm below the heads is (d, -d) on identical rows, so every weight gradient below
    them and every conv BatchNorm gradient is 0 in exact arithmetic.  Those tensors are not compared here: on the MI355X they are
    conv1_w 3.7e-3 at C = 128 and 1.9e-3 at C = 512, against a largest gradient of 0.46.  That residue is ROUNDING, not a kernel:
    tests/test_train_layers_gpu.py::test_zero_variance_batchnorm_kernel_by_kernel compares every kernel of this very step, element for
    element, with a float64 reference computed from the kernel's own device inputs, and every one meets its derived bound (worst
    err / bound at C = 128 / 512: forward GEMMs 0.053 / 0.053, wgrad 0.39 / 0.46, dgrad 0.006 / 0.006, BatchNorm backward dz 0.60 /
    0.64, and 0.998 for the f32 rounding of an FC dbeta, which is what that bound is).  Where the residue comes from: the two
    zero-variance FC BatchNorms multiply the backward signal by gamma / sqrt(eps) ~ 31.6 each, so dz is (d, -d) with |d| up to 4.6
    (fc2), 121 (fc1), 368 (conv4) and 3.2e3 (conv1) at C = 128 where an ordinary step has 1e-3 -- and every sum below is an exact 0
    obtained by cancelling such terms.  The two boards' dz add up to 0 exactly at fc1, to 3.1e-5 at conv4 and 4.4e-3 at conv1: a few
    ulp of |d| (1.4e-6 relative at conv1).  conv1's wgrad of THAT dz is 3.74e-3 in float64 and 3.72e-3 on the device (error 3.2e-4,
    bound 8.3e-2): the kernel reproduces the residue it is handed.  The losses and the tensors with a non-zero reference (FC BatchNorm,
    heads) meet the usual bars."""
    e = _engine(engine_mod, C)
    try:
        p = perturbed_params(e, 1, seed=9000 + C, C=C)
        boards, pis, vs = _identical_rows(C)
        e.train_begin(1)
        (lp, lv), g = e.train_step(boards, pis, vs, apply=False, want_grads=True)
        rlp, rlv, rg, _ = step_reference(p, C, boards, pis, vs)
        assert abs(lp - rlp) <= 1e-5 * max(1, abs(rlp)) and abs(lv - rlv) <= 1e-5 * max(1, abs(rlv)), (lp, rlp, lv, rlv)
        scale = np.abs(rg).max()
        for k, (o, shp) in layout(C)[0].items():
            n = int(np.prod(shp))
            a, r = g[o:o + n].astype(np.float64), rg[o:o + n]
            if k.endswith("_bn"):
                a, r = a[:2 * shp[1]], r[:2 * shp[1]]
            assert np.isfinite(a).all(), (C, k)
            if np.abs(r).max() > 1e-9 * scale:                        # not zero in exact arithmetic
                err = np.linalg.norm(a - r) / np.linalg.norm(r)
                assert err <= 1e-3, (C, k, err)
        p = _zero_conv3_channel(e, C, seed=9100 + C)
        boards, pis, vs = make_batch(64, seed=9200 + C)
        check_step(e, p, C, boards, pis, vs, f"C={C} b=64 constant conv3 channel")
    finally:
        e.close()


# ---- az_net_train at the bounds ------------------------------------------------------------------------------------------------------

def _replay(e, boards, pis, vs, batch, epochs, seed, src, dst):
    """test_az_net_train_is_the_documented_sequence_of_steps's replay: the steps az_net_train takes, through az_net_train_step."""
    n = boards.shape[0]

    def draw(t, j):
        r = int(mix64(np.uint64(seed)))
        for x in (t, j, 4):
            r = int(mix64(np.uint64(r ^ x)))
        return (r * n) >> 64
    key = int(mix64(np.uint64(seed ^ 0xD6E8FEB86659FD93)))
    e.train_begin(src)
    for t in range(epochs * (n // batch)):
        idx = np.array([draw(t, j) for j in range(batch)])
        e.train_step(boards[idx], pis[idx], vs[idx], mask_seed=int(mix64(np.uint64(key ^ t))), apply=True)
    e.train_end(dst)
    return e.net_get_params(dst)


@pytest.mark.parametrize("batch", [256, 100])
def test_az_net_train_replays_at_the_batch_bounds(e512, batch):
    """az_net_train (trainer_run_epoch: k_step_advance, k_gather_col1, the captured graph) at C = 512 with the largest batch and with one
    that is not a multiple of 16 (no gathered GEMMs): bit-identical to the documented sequence of az_net_train_step calls, with the
    graph and with direct launches, dropout on."""
    _restore(e512)
    n, epochs, seed = 2 * batch, 2, 4321
    boards, pis, vs = make_batch(n, seed=77 + batch)
    e512.net_init_random(8, seed=3)
    # the module's engine is shared: a step session that an earlier test left open (a second az_net_train_begin restarts it) is closed
    # here, since az_net_train is refused while one is open; id 9 is overwritten below
    e512.train_begin(8)
    e512.train_end(9)
    e512.set_option("train_dropout_e6", 300000)
    for key, val in (("train_epochs", epochs), ("train_batch", batch), ("train_seed", seed)):
        e512.set_option(key, val)
    try:
        e512.train(8, 9, boards, pis, vs)
        got = e512.net_get_params(9)
        e512.set_option("train_graph", 0)
        e512.train(8, 10, boards, pis, vs)
        assert np.array_equal(got, e512.net_get_params(10))
        assert np.isfinite(got).all()
        assert np.array_equal(got, _replay(e512, boards, pis, vs, batch, epochs, seed, 8, 11))
    finally:
        _restore(e512)


# ---- the f16 x 3 forward's range -----------------------------------------------------------------------------------------------------

def _bn_slice(C, name):
    o, shp = layout(C)[0][name]
    return o, shp[1]


def _large_beta(e, layer):
    p = perturbed_params(e, 1, seed=64, C=512)
    o, c = _bn_slice(512, f"conv{layer}_bn")
    p[o + c + 5] = 1500.0                   # beta of channel 5: every row of it enters the next conv at ~1500
    e.net_set_params(1, p)
    return p, make_batch(64, seed=164)


def _one_outlier(e):
    """The realistic mechanism: a conv1 channel that sees only the centre tap of plane 0, a batch in which one board has a stone on
    plane 0 (the others on plane 1 only), gamma = 30 on that channel.  One row of its pre-activation differs from the other 2687, so
    xhat there is ~sqrt(2687) ~ 52 and the activation ~1500: above 65504 / 64."""
    p = perturbed_params(e, 1, seed=64, C=512)
    ch = 3
    o, shp = layout(512)[0]["conv1_w"]
    w = p[o:o + int(np.prod(shp))].reshape(shp)      # [3][3][2][C]
    w[..., ch] = 0.0
    w[1, 1, 0, ch] = 8.0                             # large enough that the batch variance dwarfs eps = 1e-3
    ob, c = _bn_slice(512, "conv1_bn")
    p[ob + ch] = 30.0
    e.net_set_params(1, p)
    boards, pis, vs = make_batch(64, seed=164)
    boards[:, 1] = np.maximum(boards[:, 1], boards[:, 0])
    boards[:, 0] = 0.0
    boards[17, 1, 5, 3] = 0.0
    boards[17, 0, 5, 3] = 1.0
    return p, (boards, pis, vs)


@pytest.mark.parametrize("case", ["beta_conv1", "beta_conv2", "beta_conv3", "one_outlier"])
def test_f16x3_forward_range(e512, case):
    """Post-BatchNorm activations above 1024 entering the f16 x 3 forward (C = 512, b = 64).  With a fixed operand scale of 64 they
    overflowed half precision and the step's loss was NaN (measured on the MI355X before the fix: all four cases); the scale s_l is now
    chosen per layer from gamma, beta and the row count (act_scales_body).  The default set must give a finite step, the losses of
    float64 autograd to 1e-5, and agree with the f32 set (losses to 5e-5).
    The gradient bar here is 5e-2, not 1e-3: these inputs are ill-conditioned for ANY float32 arithmetic.  An activation of 1500 in a
    channel makes the next conv's pre-activation a large common term that its BatchNorm subtracts again, and the batch of (b) has many
    identical rows, so one ReLU flip cuts a whole group of them.  Measured worst per-tensor error against float64 autograd (MI355X;
    plain float32 PyTorch on the CPU in brackets): beta_conv1 default 7.9e-3, f32 set 3.3e-2 (7.7e-3); beta_conv2 5.2e-3, 9.5e-3
    (5.9e-3); one_outlier 1.8e-3 in every set (1.8e-3).  A wrong power of two or a NaN is off by O(1).  The moving averages are not
    compared: the batch means behind a channel at 1500 carry the same cancellation (measured 1.9e-6 off in conv4's, bar 1e-6)."""
    _restore(e512)
    p, (boards, pis, vs) = _one_outlier(e512) if case == "one_outlier" else _large_beta(e512, int(case[-1]))
    try:
        (lp, lv), g, _ = check_step(e512, p, 512, boards, pis, vs, f"C=512 b=64 {case} default", tol=5e-2, stats=False)
        e512.net_set_params(1, p)
        e512.set_option("train_gemm", 0)
        e512.train_begin(1)
        (lp32, lv32), g32 = e512.train_step(boards, pis, vs, apply=False, want_grads=True)
        assert np.isfinite(g32).all()
        # the f32 set's own loss is 1.5e-5 from float64 in beta_conv2 (measured): the two sets agree to 5e-5
        assert abs(lp - lp32) <= 5e-5 * max(1, abs(lp32)) and abs(lv - lv32) <= 5e-5 * max(1, abs(lv32)), (lp, lp32, lv, lv32)
    finally:
        _restore(e512)
