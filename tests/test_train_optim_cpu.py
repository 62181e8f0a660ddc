"""The opt-in optimiser rules of NNet::train without a GPU: csrc/az_optim.h compiled by g++ alone (tests/cpp/optim_twin.cpp) against the
float64 restatement tests/optim_ref.py -- the learning-rate schedule, the clip factor, which parameters decay --, once more under
AddressSanitizer and UBSan as a stand-alone program, and the documentation and host surfaces of the seven keys."""
import os
import re
import subprocess

import numpy as np
import pytest

import optim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("train_weight_decay_e9", "train_clip_norm_e6", "train_lr_warmup_steps", "train_lr_decay", "train_lr_floor_e6", "train_lr_total_steps",
        "train_ema_decay_e9")
FIELDS = ("weight_decay", "clip_norm", "lr_warmup_steps", "lr_decay", "lr_floor", "ema_decay")


def build_twin(out_dir, flags=()):
    exe = os.path.join(out_dir, "optim_twin" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "optim_twin.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def twin_lines(tmp_path_factory):
    exe = build_twin(str(tmp_path_factory.mktemp("optim_twin")))
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def f64(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def test_schedule_matches_the_reference(twin_lines):
    """optim_lr over warm-up 0 / 1 / 7, totals 0 / 1 / 20 / 5 (shorter than the warm-up of 7), the three modes, floors 0 / 0.1 / 1 and t up
    to 26 (beyond every total): the f32 bits of the float64 restatement for no decay and the linear mode, within 1 ulp for the cosine mode
    (libm's cos is not pinned)."""
    rows = [tuple(int(x) for x in l.split()[1:]) for l in twin_lines if l.startswith("lr ")]
    assert len(rows) == 3 * 4 * 3 * 3 * 26
    assert {(w, tot) for w, tot, *_ in rows} == {(w, tot) for w in (0, 1, 7) for tot in (0, 1, 20, 5)}
    worst = 0
    for w, total, mode, floor_e6, t, bits in rows:
        want = int(np.array([optim_ref.lr_at(np.float32(1000000 * 1e-9), t, w, total, mode, floor_e6 / 1e6)], np.float32).view(np.uint32)[0])
        d = abs(bits - want)                                   # positive floats: the bit patterns are ordered as the values
        worst = max(worst, d)
        assert d <= (1 if mode == optim_ref.COSINE else 0), (w, total, mode, floor_e6, t, f32(bits), f32(want))
    print("largest cosine deviation in ulps:", worst)
    # spot values: the warm-up's first step, the schedule's last step, beyond it
    lr = np.float32(1e-3)
    assert optim_ref.lr_at(lr, 1, 7, 20, 1, 0.1) == np.float32(float(lr) * (1 / 7))
    assert optim_ref.lr_at(lr, 20, 7, 20, 2, 0.1) == optim_ref.lr_at(lr, 26, 7, 20, 2, 0.1) == np.float32(float(lr) * 0.1)
    assert optim_ref.lr_at(lr, 3, 0, 0, 1, 0.1) == lr


def test_clip_scale_matches_the_reference(twin_lines):
    rows = [tuple(int(x) for x in l.split()[1:]) for l in twin_lines if l.startswith("clip ")]
    assert len(rows) == 4 * 12
    seen = set()
    for nb, cb, sb in rows:
        norm, c, got = f64(nb), f64(cb), f32(sb)
        want = optim_ref.clip_scale(norm, c)
        assert (np.isnan(got) and np.isnan(want)) or got == want, (norm, c, got, want)
        seen.add("nan" if np.isnan(got) else ("one" if got == 1 else "below"))
        if np.isfinite(norm):
            assert (got == 1) == (c / (norm + 1e-6) >= 1 - 2.0 ** -25), (norm, c, got)     # f32 rounding of a ratio just under 1 gives 1
    assert seen == {"nan", "one", "below"}


@pytest.mark.parametrize("C", [128, 512])
def test_decay_mask_matches_the_reference(twin_lines, C):
    rows = [tuple(int(x) for x in l.split()[1:]) for l in twin_lines if l.startswith(f"seg {C} ")]
    decays, trainable = optim_ref.masks(C)
    got = {i: (bool(d), bool(t)) for _, i, d, t in rows}
    assert set(got) == set(optim_ref.segment_edges(C))           # both edges of every segment, the layout's own offsets
    for i, (d, t) in got.items():
        assert (d, t) == (bool(decays[i]), bool(trainable[i])), (C, i)
    off = optim_ref.layout(C)[0]
    assert off["v_w"][0] % 4 == 3 and off["v_b"][0] % 4 == 3      # behind pi_b's 7 floats no boundary is 16-byte aligned: a float4 straddles them
    assert got[decays.size - 1] == (False, True) and got[decays.size - 2] == (True, True)      # v_b behind v_w


def test_twin_is_clean_under_the_sanitizers(tmp_path, twin_lines):
    """The same stand-alone program with -fsanitize=address,undefined: no report, the same output."""
    exe = build_twin(str(tmp_path), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.splitlines() == twin_lines


def test_keys_are_documented_and_the_hosts_have_the_fields():
    hdr = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    for k in KEYS:
        assert f'"{k}"' in hdr, k
    block = hdr[hdr.index("optimiser rules"):hdr.index("libaz_engine_diag.so")]
    for word in ("on ", "where ", "refused ", "purity ", "unmeasured"):
        assert word in block, word
    for f in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "train_ema_decay_e9" in open(os.path.join(ROOT, f)).read(), f
    hpp = open(os.path.join(ROOT, "include", "az_host.hpp")).read()
    cpy = open(os.path.join(ROOT, "alphazero-rs_amd", "coach.py")).read()
    for f in FIELDS:
        assert re.search(r"\b(double|int64_t)\b[^;]*\b%s\b" % f, hpp), f
        assert re.search(r"self\.%s\b" % f, cpy), f
    ex = open(os.path.join(ROOT, "examples", "connect_four.py")).read()
    for flag in ("--weight-decay", "--clip-norm", "--lr-schedule", "--ema"):
        assert flag in ex, flag
