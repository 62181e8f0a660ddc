"""The step plan of NNet::train (csrc/az_train_plan.h: which kernel chain every layer takes under the seven route switches and the shape)
as its g++ build (tests/cpp/train_plan_twin.cpp) behind ctypes, with the names of its flat int32 encoding -- the encoding the diagnostic
library's az_diag_train_plan writes as well.  The independent restatement it is held to is in tests/test_train_plan_cpu.py.  TEST
INFRASTRUCTURE ONLY.  The library is compiled once per process into a temporary directory."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCHES = ("train_gemm", "train_fwd_dma", "train_fwd_x3", "train_wgrad_tr", "train_implicit", "train_gemm3_ring", "train_fork")
DEFAULTS = {"train_gemm": 1, "train_fwd_dma": 1, "train_fwd_x3": 1, "train_wgrad_tr": 1, "train_implicit": 1, "train_gemm3_ring": 1, "train_fork": 0}

# the encoding: five step fields, then per layer eight fields and three GEMMs of five ints
STEP_FIELDS = ("x3", "fork", "perm_conv2", "split", "prep")
LAYER_FIELDS = ("fwd", "bn_small", "bn_extra", "im2col", "wgrad", "dgrad", "dgrad_dst", "col2im")
GEMMS = ("fwd_gemm", "wgrad_gemm", "dgrad_gemm")
GEMM_FIELDS = ("kernel", "M", "N", "K", "side_ws")
PER_LAYER = len(LAYER_FIELDS) + len(GEMMS) * len(GEMM_FIELDS)
INTS = len(STEP_FIELDS) + 6 * PER_LAYER

KERNEL = ("none", "gemm_f32_64", "gemm_f32_128", "gemm_f32_dma", "gemm3", "gemm3_ring", "wgrad3_tr")
FWD = ("f32", "x3_col", "x3_gather")
WGRAD = ("f32", "tr_gather", "tr_act", "tr_col", "transpose")
DGRAD = ("none", "f32", "x3", "x3_gather")
DST = ("none", "dact", "dcol")
SPLIT = ("none", "in_prep", "side_start", "after_heads")
PREP = ("none", "one", "two")
BN_OUT = {1: "f16", 2: "bf16"}
COL = {1: "f32", 2: "f16", 4: "bf16"}


def col(name, l=None, gemm=None):
    """Index of a field in the flat plan: a step field, layer l's field, or field `name` of layer l's GEMM `gemm`."""
    if l is None:
        return STEP_FIELDS.index(name)
    base = len(STEP_FIELDS) + l * PER_LAYER
    if gemm is None:
        return base + LAYER_FIELDS.index(name)
    return base + len(LAYER_FIELDS) + GEMMS.index(gemm) * len(GEMM_FIELDS) + GEMM_FIELDS.index(name)


_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="train_plan_twin_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libtrain_plan_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cpp", "train_plan_twin.cpp"), "-o", so])
        L = C.CDLL(so)
        vp = C.c_void_p
        L.twin_plan_ints.restype = C.c_int
        L.twin_train_plans.restype = None; L.twin_train_plans.argtypes = [C.c_int64, vp, vp]
        L.twin_gemm_splits.restype = None; L.twin_gemm_splits.argtypes = [C.c_int64, vp, C.c_int64, C.c_int64, vp]
        L.twin_splitk_pick.restype = None; L.twin_splitk_pick.argtypes = [C.c_int64, vp, vp]
        assert L.twin_plan_ints() == INTS
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def rows_of(cases):
    """[(C, b, {switch: value}, side stream exists)] -> the [n][10] int32 rows the twin takes (switches in SWITCHES order, side, b, C)."""
    return np.array([[{**DEFAULTS, **sw}[k] for k in SWITCHES] + [int(bool(side)), b, Cw] for Cw, b, sw, side in cases], np.int32).reshape(-1, 10)


def plans(rows):
    """The header's plans for rows [n][10] -> [n][INTS] int32."""
    rows = np.ascontiguousarray(rows, np.int32).reshape(-1, 10)
    out = np.zeros((len(rows), INTS), np.int32)
    lib().twin_train_plans(len(rows), _p(rows), _p(out))
    return out


def gemm_splits(gemms, ws_main, ws_side):
    """GEMMs [n][5] as encoded -> [n][4]: K-steps, slices wanted, steps per slice, slices (zeros where the kernel is none)."""
    gemms = np.ascontiguousarray(gemms, np.int32).reshape(-1, 5)
    out = np.zeros((len(gemms), 4), np.int32)
    lib().twin_gemm_splits(len(gemms), _p(gemms), int(ws_main), int(ws_side), _p(out))
    return out


def splitk_pick(args):
    """[n][4] int64 (steps, want, out_elems, ws_floats) -> [n][2]: steps per slice, slices."""
    args = np.ascontiguousarray(args, np.int64).reshape(-1, 4)
    out = np.zeros((len(args), 2), np.int32)
    lib().twin_splitk_pick(len(args), _p(args), _p(out))
    return out


def _set(bits, names):
    return frozenset(n for v, n in names.items() if bits & v)


def decode(flat):
    """One flat plan -> {"x3", "fork", "perm_conv2": bool, "split", "prep": names, "layers": six dicts with the routes by name, "bn": "small"
    / "large", "bn_extra" and "im2col" as sets of formats (im2col None where the kernel is not launched), the three GEMMs' kernel names}."""
    f = [int(v) for v in flat]
    out = {"x3": bool(f[0]), "fork": bool(f[1]), "perm_conv2": bool(f[2]), "split": SPLIT[f[3]], "prep": PREP[f[4]], "layers": []}
    for l in range(6):
        g = lambda name: f[col(name, l)]
        out["layers"].append({
            "fwd": FWD[g("fwd")], "bn": "small" if g("bn_small") else "large", "bn_extra": _set(g("bn_extra"), BN_OUT),
            "im2col": _set(g("im2col"), COL) if g("im2col") else None, "wgrad": WGRAD[g("wgrad")], "dgrad": DGRAD[g("dgrad")],
            "dst": DST[g("dgrad_dst")], "col2im": bool(g("col2im")),
            **{k + "_kernel": KERNEL[f[col("kernel", l, k + "_gemm")]] for k in ("fwd", "wgrad", "dgrad")}})
    return out


def plan(Cw, b, switches={}, side=False):
    return decode(plans(rows_of([(Cw, b, switches, side)]))[0])
