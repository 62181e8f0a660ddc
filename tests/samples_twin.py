"""The window check of csrc/az_samples.h -- what every entry that takes an az_samples refuses in a tuple, and the sentences it refuses
with -- as its g++ build (tests/cpp/samples_twin.cpp) behind ctypes.  The independent restatements it is held to are merge_twin.refusal
and mirror_twin.boards_to_states.  TEST INFRASTRUCTURE ONLY.  The library is compiled once per process into a temporary directory
(g++ -O2 -ffp-contract=off, the flags the header states)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_VALUE, BAD_STATE, BAD_FEATURE, BAD_PRIOR = 1, 2, 4, 8

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="samples_twin_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libsamples_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "samples_twin.cpp"), "-o", so])
        L = C.CDLL(so)
        vp = C.c_void_p
        L.twin_sample_check.restype = C.c_uint32; L.twin_sample_check.argtypes = [C.c_int64, vp, vp, vp, vp, C.c_int32, vp, vp]
        L.twin_sample_bad_text.restype = C.c_char_p; L.twin_sample_bad_text.argtypes = [C.c_uint32, C.c_int32]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(pis, zs, *, states=None, boards=None, strict_pi=False):
    """(verdict word, bits [n] u32, states [n,2] u64 as the check saw them) of a window on the states or the boards route."""
    pis = np.ascontiguousarray(pis, np.float32).reshape(-1, 7)
    n = len(pis)
    zs = np.ascontiguousarray(zs, np.float32).reshape(n)
    states = None if states is None else np.ascontiguousarray(states, np.uint64).reshape(n, 2)
    boards = None if boards is None else np.ascontiguousarray(boards, np.float32).reshape(n, 84)
    bits, seen = np.zeros(n, np.uint32), np.zeros((n, 2), np.uint64)
    word = lib().twin_sample_check(n, _p(states), _p(boards), _p(pis), _p(zs), int(bool(strict_pi)), _p(bits), _p(seen))
    return int(word), bits, seen


def bad_text(bits, strict_pi=False):
    t = lib().twin_sample_bad_text(int(bits), int(bool(strict_pi)))
    return None if t is None else t.decode()
