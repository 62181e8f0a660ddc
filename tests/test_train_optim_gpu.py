"""The opt-in optimiser rules of NNet::train on the device ("train_weight_decay_e9", "train_clip_norm_e6", "train_lr_warmup_steps",
"train_lr_decay", "train_lr_floor_e6", "train_lr_total_steps", "train_ema_decay_e9"; csrc/az_optim.h, k_grad_sqnorm and k_adamw in
csrc/az_train.hip) against the float64 restatement tests/optim_ref.py, through the C ABI.  C = 128 (the smallest width; v_w and v_b are
not 16-byte aligned at any width), batch 32, 5 applied steps, dropout off, test_train_gpu.py's perturbed weights."""
import os
import subprocess

import numpy as np
import pytest

import optim_ref
from test_train_gpu import make_batch, perturbed_params, set_gemms
from train_ref import mix64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C = 128
KEYS = ("train_weight_decay_e9", "train_clip_norm_e6", "train_lr_warmup_steps", "train_lr_decay", "train_lr_floor_e6", "train_lr_total_steps",
        "train_ema_decay_e9")
ALL_ON = dict(weight_decay=0.1, lr_warmup_steps=2, lr_decay=1, lr_floor=0.1, lr_total_steps=5, ema_decay=0.9)


@pytest.fixture(scope="module")
def oengine(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=1024, net_channels=C)
    e.set_option("train_dropout_e6", 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """tests/cpp/optim_twin.cpp: the schedule as the engine's host code computes it (the same libm cos)."""
    exe = os.path.join(str(tmp_path_factory.mktemp("optim_twin")), "optim_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "optim_twin.cpp"), "-o", exe])

    def table(steps, warmup, total, mode, floor_e6, lr_e9=1000000):
        out = subprocess.run([exe, "lr", str(lr_e9), str(steps), str(warmup), str(total), str(mode), str(floor_e6)], check=True,
                             stdout=subprocess.PIPE, text=True).stdout.split()
        return np.array([int(x) for x in out], np.uint32).view(np.float32)
    return table


def run_steps(e, src, dst, batches, want_grads=True, ema_dst=None, **optim):
    """train_begin(src) under the given rules, one applied step per batch, train_end(dst) -> (weights, [grads], [step info], ema weights);
    the rules are back at their defaults afterwards."""
    e.set_train_optim(**optim)
    try:
        e.train_begin(src)
        grads, info = [], []
        for bt in batches:
            _, g = e.train_step(*bt, apply=True, want_grads=want_grads)
            grads.append(g)
            info.append(e.train_step_info())
        e.train_end(dst)
        ema = None
        if ema_dst is not None:
            e.train_ema(ema_dst)
            ema = e.net_get_params(ema_dst)
        return e.net_get_params(dst), grads, info, ema
    finally:
        e.set_train_optim()


@pytest.fixture(scope="module")
def baseline(oengine):
    """The five steps with every rule off: starting weights, batches, final weights, the raw gradients' float64 norms."""
    p = perturbed_params(oengine, 3, seed=11)
    batches = [make_batch(32, seed=200 + i) for i in range(5)]
    got, grads, info, _ = run_steps(oengine, 3, 4, batches)
    assert all(i == (-1.0, 1.0, float(np.float32(1e-3)), t) for t, i in enumerate(info, start=1)), info
    norms = [float(np.sqrt(np.sum(g.astype(np.float64) ** 2))) for g in grads]
    return p, batches, got, norms


REPLAYS = {"weight_decay": dict(weight_decay=0.1), "clip": dict(), "schedule": dict(lr_warmup_steps=2, lr_decay=1, lr_floor=0.1, lr_total_steps=5),
           "linear_schedule": dict(lr_warmup_steps=1, lr_decay=2, lr_floor=0.25, lr_total_steps=4), "ema": dict(ema_decay=0.9), "all": dict(ALL_ON)}


@pytest.mark.parametrize("name", list(REPLAYS))
def test_update_replays_from_the_device_gradients(oengine, baseline, name):
    """test_train_gpu.py's test_adam_update_replays_from_the_device_gradients for the new rule: the RAW gradients the device reports,
    fed into optim_ref.replay in float64, reproduce the device's final weights and the averaged model to 1e-6 on every trainable slot
    (now two f32 roundings of a parameter <= 1.5 per step -- the decay and the update: ten half-ulps of 1.2e-7 = 6e-7).  wd = 0.1
    makes a wrongly decayed gamma, or a wrongly skipped weight, miss by 5e-4.  Measured: weights 2.6e-7 or less, averaged model 3.0e-7 or
    less, in all six cases."""
    p, batches, _, norms = baseline
    optim = dict(REPLAYS[name])
    if name in ("clip", "all"):
        optim["clip_norm"] = int(round(float(np.median(norms)) * 1e6)) / 1e6      # a value the key carries exactly
    ema_on = optim.get("ema_decay", 0) > 0
    got, grads, info, ema = run_steps(oengine, 3, 5, batches, ema_dst=6 if ema_on else None, **optim)
    q, s, rinfo = optim_ref.replay(p, grads, C, wd=optim.get("weight_decay", 0.0), clip=optim.get("clip_norm", 0.0),
                                   warmup=optim.get("lr_warmup_steps", 0), total=optim.get("lr_total_steps", 0), mode=optim.get("lr_decay", 0),
                                   floor=optim.get("lr_floor", 0.0), ema=optim.get("ema_decay", 0.0))
    _, trainable = optim_ref.masks(C)
    err = np.abs(got.astype(np.float64) - q)[trainable].max()
    print(f"[replay] {name}: weights {err:.2e}")
    assert err <= 1e-6, err
    assert np.abs(got - p)[trainable].max() > 1e-3                       # and the weights did move
    for (norm, scale, lr_t, t), (rnorm, rscale, rlr), step in zip(info, rinfo, range(1, 6)):
        assert t == step and np.float32(lr_t) == np.float32(rlr), (step, lr_t, rlr)
        if "clip_norm" in optim:
            assert abs(norm - rnorm) <= 1e-9 * rnorm and abs(scale - rscale) <= 2.0 ** -23 * rscale, (norm, rnorm, scale, rscale)
        else:
            assert (norm, scale) == (-1.0, 1.0)
    if ema_on:
        eerr = np.abs(ema.astype(np.float64) - s)[trainable].max()
        print(f"[replay] {name}: averaged model {eerr:.2e}")
        assert eerr <= 1e-6, eerr
        assert np.array_equal(ema[~trainable], got[~trainable])          # the moving averages are the live trainer's, bit for bit
        assert np.abs(ema - got)[trainable].max() > 1e-4                 # and it is not the raw model
    else:
        with pytest.raises(Exception):
            oengine.train_ema(6)                                          # the session did not average


def test_clipping_three_passes(oengine, baseline):
    """A c no step reaches (scale exactly 1) is bit-identical to clipping off.  With c at the median of the reported norms some steps
    are clipped and some are not; the reported norm is numpy's float64 norm of the raw gradient to 1e-9 relative (n 2^-53 for the
    n = 1.8 M non-negative terms of either sum), the reported factor optim_clip_scale of it to one f32 ulp; the pass repeated gives the
    same bits."""
    p, batches, off, _ = baseline
    got1, grads1, info1, _ = run_steps(oengine, 3, 5, batches, clip_norm=1e6)
    assert np.array_equal(got1, off)
    assert all(i[1] == 1.0 for i in info1)
    c = int(round(float(np.median([i[0] for i in info1])) * 1e6)) / 1e6      # a value the key carries exactly
    got2, grads2, info2, _ = run_steps(oengine, 3, 5, batches, clip_norm=c)
    scales = [i[1] for i in info2]
    assert any(s < 1.0 for s in scales) and any(s == 1.0 for s in scales), scales
    assert not np.array_equal(got2, off)
    for infos, grads in ((info1, grads1), (info2, grads2)):
        for (norm, scale, _, _), g in zip(infos, grads):
            ref = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
            print(f"[clip] norm {norm:.12g} (numpy {ref:.12g}, rel {abs(norm - ref) / ref:.1e}) scale {scale:.9g}")
            assert abs(norm - ref) <= 1e-9 * ref, (norm, ref)
            want = float(optim_ref.clip_scale(norm, 1e6 if infos is info1 else c))
            assert abs(scale - want) <= 2.0 ** -23 * want, (scale, want)
    got3, grads3, info3, _ = run_steps(oengine, 3, 6, batches, clip_norm=c)
    assert np.array_equal(got3, got2) and info3 == info2
    assert all(np.array_equal(a, b) for a, b in zip(grads3, grads2))


def test_az_net_train_is_the_documented_sequence_of_steps_with_every_rule_on(oengine, twin):
    """az_net_train with every rule on = the hand replay through az_net_train_step on the documented batches and mask seeds with
    "train_lr_total_steps" = epochs x steps, bit for bit, weights and averaged model: the captured graph (the schedule table indexed on
    the device) and direct launches, "train_fork" 1 included.  lr_t of every step is the twin's table (the host's own cos)."""
    e = oengine
    n, batch, epochs, seed = 256, 32, 2, 1234
    steps = epochs * (n // batch)
    boards, pis, vs = make_batch(n, seed=77)
    perturbed_params(e, 8, seed=3)
    optim = dict(ALL_ON, lr_total_steps=0)
    for key, val in (("train_epochs", epochs), ("train_batch", batch), ("train_seed", seed)):
        e.set_option(key, val)
    try:
        e.train_begin(8)
        _, g = e.train_step(boards[:batch], pis[:batch], vs[:batch], apply=False, want_grads=True)
        optim["clip_norm"] = float(np.sqrt(np.sum(g.astype(np.float64) ** 2))) * 0.8
        e.train_end(9)
        got = {}
        for graph, fork in ((1, 0), (0, 0), (1, 1), (0, 1)):
            e.set_option("train_graph", graph)
            e.set_option("train_fork", fork)
            e.set_train_optim(**optim)
            e.train(8, 9, boards, pis, vs)
            e.set_train_optim()
            e.train_ema(10)
            got[graph, fork] = (e.net_get_params(9), e.net_get_params(10), e.train_step_info())
        e.set_option("train_graph", 1)
        e.set_option("train_fork", 0)
        ref = got[1, 0]
        for k, v in got.items():
            assert np.array_equal(v[0], ref[0]) and np.array_equal(v[1], ref[1]) and v[2] == ref[2], k
        table = twin(steps, 2, steps, 1, 100000)
        assert np.float32(ref[2][2]) == table[-1] and ref[2][3] == steps

        def draw(t, j):
            r = int(mix64(np.uint64(seed)))
            for x in (t, j, 4):
                r = int(mix64(np.uint64(r ^ x)))
            return (r * n) >> 64
        key = int(mix64(np.uint64(seed ^ 0xD6E8FEB86659FD93)))
        e.set_train_optim(**dict(optim, lr_total_steps=steps))
        e.train_begin(8)
        e.set_train_optim()
        clipped = []
        for t in range(steps):
            idx = np.array([draw(t, j) for j in range(batch)])
            e.train_step(boards[idx], pis[idx], vs[idx], mask_seed=int(mix64(np.uint64(key ^ t))), apply=True)
            norm, scale, lr_t, applied = e.train_step_info()
            assert np.float32(lr_t) == table[t] and applied == t + 1, (t, lr_t, table[t])
            clipped.append(scale < 1.0)
        e.train_end(11)
        e.train_ema(12)
        assert any(clipped)
        assert np.array_equal(ref[0], e.net_get_params(11))
        assert np.array_equal(ref[1], e.net_get_params(12))
        assert e.train_step_info() == ref[2]
        # the reference's table: exact where no cos is involved, one ulp where it is
        rt = optim_ref.lr_table(1e-3, steps, 2, steps, 1, 0.1)
        assert np.abs(table.view(np.int32) - rt.view(np.int32)).max() <= 1
    finally:
        e.set_train_optim()
        e.set_option("train_graph", 1)
        e.set_option("train_fork", 0)
        for key, val in (("train_epochs", 10), ("train_batch", 64), ("train_seed", 0)):
            e.set_option(key, val)


@pytest.mark.parametrize("gemm_set", [(1, 1, 1), (0, 1, 0)], ids=["default", "f32_gemms"])
def test_an_engine_back_at_the_defaults_trains_the_bits_of_a_fresh_one(engine_mod, gemm_set):
    n, batch = 128, 32
    boards, pis, vs = make_batch(n, seed=5)
    got = []
    for touched in (True, False):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=C)
        try:
            set_gemms(e, gemm_set)
            for key, val in (("train_epochs", 2), ("train_batch", batch), ("train_seed", 7)):
                e.set_option(key, val)
            e.net_init_random(1, seed=2)
            if touched:
                e.set_train_optim(clip_norm=0.5, **dict(ALL_ON, lr_total_steps=3))
                e.train(1, 2, boards, pis, vs)
                e.train_ema(3)
                with_rules = e.net_get_params(2)
                e.set_train_optim()
            e.train(1, 2, boards, pis, vs)
            got.append(e.net_get_params(2))
            assert e.train_step_info()[:2] == (-1.0, 1.0)
            with pytest.raises(Exception):
                e.train_ema(3)                                           # that session did not average
        finally:
            e.close()
    assert np.array_equal(got[0], got[1])
    assert not np.array_equal(with_rules, got[0])


def test_refusals(engine_mod):
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=C)
    try:
        bad = {"train_weight_decay_e9": (-1, 10 ** 9 + 1), "train_clip_norm_e6": (-1, 10 ** 12 + 1), "train_lr_warmup_steps": (-1, 2 ** 31),
               "train_lr_decay": (-1, 3), "train_lr_floor_e6": (-1, 10 ** 6 + 1), "train_lr_total_steps": (-1, 2 ** 31),
               "train_ema_decay_e9": (-1, 10 ** 9)}
        good = {"train_weight_decay_e9": (0, 10 ** 9), "train_clip_norm_e6": (0, 1, 10 ** 12), "train_lr_warmup_steps": (0, 2 ** 31 - 1),
                "train_lr_decay": (0, 1, 2), "train_lr_floor_e6": (0, 10 ** 6), "train_lr_total_steps": (0, 2 ** 31 - 1),
                "train_ema_decay_e9": (0, 1, 10 ** 9 - 1)}
        assert set(bad) == set(good) == set(KEYS)
        for k in KEYS:
            for v in bad[k]:
                with pytest.raises(engine_mod.AzError) as ex:
                    e.set_option(k, v)
                assert ex.value.status == 1, (k, v)                      # AZ_ERR_BAD_ARGUMENT
            for v in good[k]:
                e.set_option(k, v)
            e.set_option(k, 0)
        with pytest.raises(engine_mod.AzError) as ex:
            e.train_step_info()                                           # no training yet
        assert ex.value.status == 1
        with pytest.raises(engine_mod.AzError) as ex:
            e.train_ema(2)                                                # no training yet
        assert ex.value.status == 1
        e.net_init_random(1, seed=0)
        bt = make_batch(8, seed=1)
        e.train_begin(1)                                                  # a session with the key at 0
        e.train_step(*bt)
        with pytest.raises(engine_mod.AzError) as ex:
            e.train_ema(2)
        assert ex.value.status == 1
        e.train_end(2)
        e.set_option("train_ema_decay_e9", 900000000)
        e.train_begin(1)
        e.set_option("train_ema_decay_e9", 0)                             # the session keeps what its begin saw
        e.train_step(*bt)
        e.train_ema(3)                                                    # between begin and end
        mid = e.net_get_params(3)
        e.train_step(*bt, apply=False)                                    # apply = 0 does not move the shadow
        e.train_end(2)
        e.train_ema(3)                                                    # and after end
        _, trainable = optim_ref.masks(C)
        assert np.array_equal(mid[trainable], e.net_get_params(3)[trainable])
        e.train_begin(1)                                                  # the next begin, the key at 0 again
        with pytest.raises(engine_mod.AzError) as ex:
            e.train_ema(3)
        assert ex.value.status == 1
        e.train_end(2)
    finally:
        e.close()
