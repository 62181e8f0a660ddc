"""The two Coaches with the optimiser rules of NNet::train on (Coach.weight_decay / clip_norm / lr_warmup_steps / lr_decay / lr_floor /
ema_decay in coach.py and include/az_host.hpp): one iteration of tests/test_coach_gpu.py::test_python_and_cpp_coach_agree in miniature
on both hosts -- same report, byte-identical files --, the keys on around the one az_net_train only, the candidate the averaged model."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg        # noqa: E402

FIELDS = dict(weight_decay=0.05, clip_norm=1.5, lr_warmup_steps=3, lr_decay=1, lr_floor=0.1, ema_decay=0.8)
KEYS = ("train_weight_decay_e9", "train_clip_norm_e6", "train_lr_warmup_steps", "train_lr_decay", "train_lr_floor_e6", "train_lr_total_steps",
        "train_ema_decay_e9")
SIMS = 16


def run_python(engine_mod, d, optim, seen=None):
    from alphazero_rs_amd.coach import Coach
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    try:
        e.net_init_random(0, 3)
        e.set_option("train_epochs", 1)
        coach = Coach.setup(e, d, 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 1, 32, SIMS, 1, 1000, 1, log=lambda m: None)
        if optim:
            for k, v in FIELDS.items():
                setattr(coach, k, v)
        if seen is not None:
            orig_set, orig_train, orig_ema, orig_arena = e.set_option, e.train, e.train_ema, e.arena

            def spy(key, value):
                if key in KEYS:
                    seen.append((key, value))
                return orig_set(key, value)

            def named(name, f):
                def call(*a, **kw):
                    seen.append((name, 0))
                    return f(*a, **kw)
                return call
            e.set_option, e.train, e.train_ema, e.arena = spy, named("train", orig_train), named("train_ema", orig_ema), named("arena", orig_arena)
        return coach.learn(seed=11)
    finally:
        e.close()


def test_python_and_cpp_coach_agree_with_the_optimiser_rules(engine_mod, tmp_path):
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp", "plain")}
    seen = []
    rep = run_python(engine_mod, dirs["py"], True, seen)
    run_python(engine_mod, dirs["plain"], False)
    exe = os.path.join(tmp_path, "test_coach_optim")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_optim.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, dirs["cpp"], "128", "11"] + [f"{k}={v}" for k, v in FIELDS.items()] + [f"num_sims={SIMS}"], check=True,
                         stdout=subprocess.PIPE, text=True, timeout=600).stdout
    crep = json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    assert len(rep) == len(crep) == 1
    for k in fg.REPORT_KEYS:
        assert rep[0][k] == crep[0][k], k
    fg.compare_directories(dirs["py"], dirs["cpp"])
    read = lambda d, f: open(os.path.join(dirs[d], f), "rb").read()
    assert read("py", "1.aznet") != read("plain", "1.aznet")                # the rules really shaped the candidate
    assert read("py", "0.examples") == read("plain", "0.examples")          # and nothing but training
    # on around the one az_net_train, off again behind it, the averaged model stored before the arena
    on = [("train_weight_decay_e9", 50000000), ("train_clip_norm_e6", 1500000), ("train_lr_warmup_steps", 3), ("train_lr_decay", 1),
          ("train_lr_floor_e6", 100000), ("train_lr_total_steps", 0), ("train_ema_decay_e9", 800000000)]
    assert seen == on + [("train", 0)] + [(k, 0) for k in KEYS] + [("train_ema", 0), ("arena", 0)], seen
