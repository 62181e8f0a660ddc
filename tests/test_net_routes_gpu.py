"""GPU tests that hold the inference forward to the layer-by-layer reference at every hand-over between two kernels, with the three
numbers a search hands the launchers given apart: n (the exact row count, read on the device), rows_hint (the host's bound: the
grids) and rows_typ (the host's estimate: the kernel families).  az_net_predict_states -- the entry every other reference test goes
through -- can only run rows_hint == n, rows_typ == 0; the diagnostic library's az_diag_predict_hinted runs ONE forward with all
three as given, fills all rows_hint rows of pi / v with a NaN sentinel first and returns all of them.

The triples come from tests/net_routes.py (both sides of every line, under every regime of (rows_hint, rows_typ) the line is live
in; tests/test_net_routes_cpu.py holds that module to the source text), at C = 512 and -- for the lines that move with the number
of column tiles -- at C = 256, on engines with max_batch = 8192.

Before every triple a DECOY forward of other states runs at the same (n, rows_hint, rows_typ), and the entry itself fills rows
[0, rows_hint) of act2 .. fc2o with NaN bytes before its forward: an element that no kernel writes reads as a NaN -- never as an
earlier triple's right answer, which a decoy alone cannot rule out (a launcher that skips some tiles at a given triple skips them
for the decoy too, and every triple forwards a prefix of the same states).

  exact data   integer parameters (net_ref.exact_params) on a pool of 8192 distinct legal states whose reference is computed once
               per width and class: layers 2 .. 6 of rows [0, n) must be the reference's bits (fp8: conv2 / conv3 codes and the
               bf16 layers behind them), pi / v within the 1e-6 left to exp / tanh and bit-equal to az_net_predict_states on the
               same states in chunks of 128, rows [n, rows_hint) of pi / v still the sentinel.  bf16: under the shipped options and
               under each of conv3_tail 0, conv3_wreg 0, conv3_planes 0, narrow_rows 0, conv3_small 0, conv2_table 0 + conv1_table 0.
               fp8: shipped and narrow_rows 0 (the other switches pick bf16 kernels only); the count of k_gemm_skinny_f8 launches
               rises by exactly what net_routes.fp8_skinny_launches says, forward by forward.
  random data  random_params: the tile choice must not change a rounding.  Layers and (pi, v) of every hinted forward are bit-equal
               to the same states forwarded through az_net_predict_states in chunks of 128 -- the size the layer tests hold to
               float64 (tests/test_net_layers_gpu.py, tests/test_net_layers_fp8_gpu.py).

No bar here is measured: bit-equality, the sentinel, and the 1e-6 of the existing exact-data tests.
"""
import ctypes

import numpy as np
import pytest
import torch

import net_layers_ref as L
import net_layers_ref_fp8 as L8
import net_routes as R
from net_ref import exact_params, random_params
from test_fp8_gpu import fp8_scales
from test_net_gpu import random_states

pytestmark = pytest.mark.gpu

MB = R.MAX_BATCH
SENTINEL = 0x7FC5A5A5                  # AZ_DIAG_HINTED_SENTINEL of csrc/az_engine.hip
CHUNK = 128
REF_CHUNK = 512                        # states per reference evaluation (memory, not meaning)
DECOY_SHIFT = 4099                     # the decoy's row i is the pool's state i + 4099: no row keeps its state
DEFAULTS = {"conv2_table": 1, "conv1_table": 1, "conv3_small": 1, "narrow_rows": 32, "conv3_wreg": 1, "conv3_planes": 1, "conv3_tail": 1}
OPTION_SETS = [{}, {"conv3_tail": 0}, {"conv3_wreg": 0}, {"conv3_planes": 0}, {"narrow_rows": 0}, {"conv3_small": 0}, {"conv2_table": 0, "conv1_table": 0}]
FP8_OPTION_SETS = [{}, {"narrow_rows": 0}]
# per board: (reader, reader's layer argument, elements, numpy dtype)
BF16_LAYERS = {"conv2": ("act", 2, lambda c: 42 * c, np.uint16), "conv3": ("act", 3, lambda c: 20 * c, np.uint16), "conv4": ("act", 4, lambda c: 6 * c, np.uint16),
               "fc1": ("act", 5, lambda c: 1024, np.uint16), "fc2": ("act", 6, lambda c: 512, np.uint16)}
FP8_LAYERS = {"act2": ("conv2_fp8", None, lambda c: 42 * c, np.uint8), "act3": ("conv3_fp8", None, lambda c: 20 * c, np.uint8), "act4": BF16_LAYERS["conv4"],
              "fc1": BF16_LAYERS["fc1"], "fc2": BF16_LAYERS["fc2"]}


def triples(channels, cls):
    return R.cases(512, cls) if channels == 512 else R.cases(channels, cls, only=R.moved_lines(channels, 512, cls))


# ---- the device side --------------------------------------------------------------------------------------------------
def hinted(e, model_id, states, rows_hint, rows_typ):
    """az_diag_predict_hinted on len(states) rows -> (pi [rows_hint][7], v [rows_hint]), or None where it refuses."""
    f = e._lib.az_diag_predict_hinted
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 2)
    pi = np.zeros((max(rows_hint, 1), 7), np.float32)
    v = np.zeros(max(rows_hint, 1), np.float32)
    got = f(e._h, model_id, s.ctypes.data_as(ctypes.c_void_p), len(s), rows_hint, rows_typ, pi.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p))
    if got == -1:
        assert not pi.any() and not v.any()               # a refusal writes nothing
        return None
    assert got == rows_hint * 32, (got, rows_hint)
    return pi, v


class Reader:
    """The layers of the engine's last forward, read into page-locked buffers that are allocated once (a fresh 350 MB array per read
    would cost more than the copy)."""

    def __init__(self, channels, layers):
        self.channels, self.layers = channels, layers
        self.buf = {name: torch.empty((MB, per(channels)), dtype=torch.int16 if dt == np.uint16 else torch.uint8, pin_memory=True)
                    for name, (_, _, per, dt) in layers.items()}

    def read(self, e, name, rows):
        kind, layer, _, _ = self.layers[name]
        out = self.buf[name][:rows]
        if kind == "act":
            f = e._lib.az_diag_read_act
            f.restype, f.argtypes = ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
            got = f(e._h, layer, rows, ctypes.c_void_p(out.data_ptr()))
        else:
            f = e._lib.az_diag_read_conv2_out_fp8 if kind == "conv2_fp8" else e._lib.az_diag_read_conv3_out_fp8
            f.restype, f.argtypes = ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
            got = f(e._h, rows, ctypes.c_void_p(out.data_ptr()))
        assert got == out.numel() * out.element_size(), (name, rows, got)
        return out


def as_tensor(a):
    """A reference array -> [rows][elements per board], in the reader's integer type."""
    a = np.ascontiguousarray(a)
    a = a.view(np.int16) if a.dtype == np.uint16 else a
    return torch.from_numpy(a.reshape(a.shape[0], -1))


def set_options(e, opts):
    for k, val in {**DEFAULTS, **opts}.items():
        e.set_option(k, val)


def chunked_predict(e, model_id, states, reader=None):
    """az_net_predict_states in chunks of 128 -> (pi, v) and, with a reader, every layer of every chunk."""
    pi = np.empty((len(states), 7), np.float32)
    v = np.empty(len(states), np.float32)
    layers = {name: torch.empty_like(buf[:len(states)], pin_memory=False) for name, buf in reader.buf.items()} if reader else None
    for o in range(0, len(states), CHUNK):
        pi[o:o + CHUNK], v[o:o + CHUNK] = e.predict_states(states[o:o + CHUNK], model_id)
        if reader:
            k = min(CHUNK, len(states) - o)
            for name in layers:
                layers[name][o:o + k] = reader.read(e, name, k)
    return pi, v, layers


def describe(got, want, channels):
    """What differs between two [rows][elements] tensors, in the words of test_exact_data_every_layer_bit_for_bit."""
    width = channels if got.shape[1] % channels == 0 and got.shape[1] > 1024 else got.shape[1]
    bad = np.argwhere((got != want).numpy().reshape(got.shape[0], -1, width))
    return ("elements that differ", len(bad), "first (board, position, channel)", bad[:4].tolist(), "boards", np.unique(bad[:, 0])[:8].tolist(),
            "channels", np.unique(bad[:, -1])[:8].tolist())


def sweep(e, model_id, channels, tag, cases, states, want_layers, want_pi, want_v, reader, ref_heads=None, fp8_narrow=None):
    """Every triple: the decoy, the forward, every layer of rows [0, n), the heads, the sentinel.  All failing triples are collected;
    the message names each with its layer (the first eight in detail)."""
    decoy = np.roll(states, -DECOY_SHIFT, axis=0)
    failures = []

    def fail(triple, *what):
        failures.append((triple,) + what if len(failures) < 8 else (triple, what[0], what[1]))

    count = e._lib.az_diag_fp8_skinny_launches
    count.restype, count.argtypes = ctypes.c_longlong, [ctypes.c_void_p]
    for triple in cases:
        n, hint, typ = triple
        before = count(e._h)
        assert hinted(e, model_id, decoy[:n], hint, typ) is not None, triple
        out = hinted(e, model_id, states[:n], hint, typ)
        assert out is not None, triple
        pi, v = out
        if fp8_narrow is not None:
            rose, expect = count(e._h) - before, 2 * R.fp8_skinny_launches(channels, hint, typ, fp8_narrow)
            if rose != expect:
                fail(triple, "k_gemm_skinny_f8 launches", rose, "expected", expect)
        for name, want in want_layers.items():
            got = reader.read(e, name, n)
            if not torch.equal(got, want[:n]):
                fail(triple, "layer", name, *(describe(got, want[:n], channels) if len(failures) < 8 else ()))
        if not (np.array_equal(pi[:n], want_pi[:n]) and np.array_equal(v[:n], want_v[:n])):
            rows = np.flatnonzero((pi[:n] != want_pi[:n]).any(axis=1) | (v[:n] != want_v[:n]))
            fail(triple, "heads", "(pi, v) rows that differ from predict_states in chunks", len(rows), "first", rows[:8].tolist())
        if ref_heads is not None:
            dp, dv = np.abs(pi[:n] - ref_heads[0][:n]).max(), np.abs(v[:n] - ref_heads[1][:n]).max()
            if not (dp <= 1e-6 and dv <= 1e-6):
                fail(triple, "heads", "against the reference", float(dp), float(dv))
        tail = np.concatenate([pi[n:].view(np.uint32).ravel(), v[n:].view(np.uint32)])
        if (tail != SENTINEL).any():
            fail(triple, "heads", "rows past n that were written", int((pi[n:].view(np.uint32) != SENTINEL).any(axis=1).sum()), "of", hint - n)
    if failures:
        raise AssertionError((f"C={channels} {tag}", "triples (n, rows_hint, rows_typ) that fail", len({f[0] for f in failures}), failures[:24]))


# ---- the pool and its references (once per module) -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(oracle):
    """16384 distinct legal states in a fixed order (random play repeats its openings: drawn until enough are distinct)."""
    seen, out, seed = set(), [], 500
    while len(out) < 2 * MB:
        for s in random_states(oracle, 4096, seed=seed):
            key = (int(s[0]), int(s[1]))
            if key not in seen and len(out) < 2 * MB:
                seen.add(key)
                out.append(key)
        seed += 1
        assert seed < 520
    st = np.array(out, dtype=np.uint64)
    assert st.shape == (2 * MB, 2) and len(np.unique(st, axis=0)) == 2 * MB and not (st[:, 0] & st[:, 1]).any()
    return st[np.random.default_rng(11).permutation(2 * MB)]


def bf16_rows_ok(ref, rpi, rv):
    """Per state: the row-wise conditions of net_layers_ref.exact_conditions (every f32 order exact, integers, unsaturated heads)."""
    n = len(rv)
    ok = (rpi.max(axis=1) < 0.999) & (np.abs(rv) < 0.999)
    for name in L.LAYERS:
        y, S, _ = ref[name]
        ok &= (S.reshape(n, -1).max(axis=1) < 2 ** 24) & (y == np.rint(y)).reshape(n, -1).all(axis=1)
    return ok


def fp8_rows_ok(ref):
    n = len(ref["v"])
    ok = (ref["pi"].max(axis=1) < 0.999) & (np.abs(ref["v"]) < 0.999)
    y2, S2 = ref["conv2"]
    ok &= (S2.reshape(n, -1).max(axis=1) < 2 ** 24) & (y2 == np.rint(y2)).reshape(n, -1).all(axis=1)
    for name in ("fc1", "fc2"):
        y, S = ref[name + "_yS"]
        ok &= (S.reshape(n, -1).max(axis=1) < 2 ** 24) & (y == np.rint(y)).reshape(n, -1).all(axis=1)
    return ok


def build_reference(pool, evaluate, layer_names):
    """The reference of the first 8192 states of the pool whose own rows meet the exact-data conditions, REF_CHUNK at a time:
    evaluate(chunk) -> (keep mask, {layer: array}, pi, v) and asserts the conditions on what it keeps.  Fails if fewer than 8192 of
    the 16384 survive."""
    states, layers, pis, vs, have = [], {k: [] for k in layer_names}, [], [], 0
    for o in range(0, len(pool), REF_CHUNK):
        keep, lay, pi, v = evaluate(pool[o:o + REF_CHUNK])
        keep &= np.cumsum(keep) <= MB - have
        states.append(pool[o:o + REF_CHUNK][keep])
        for k in layer_names:
            layers[k].append(as_tensor(lay[k][keep]))
        pis.append(pi[keep])
        vs.append(v[keep])
        have += int(keep.sum())
        if have == MB:
            break
    assert have == MB, ("states of the pool that meet the exact-data conditions", have, "of", len(pool))
    return {"states": np.concatenate(states), "layers": {k: torch.cat(layers[k]) for k in layer_names}, "pi": np.concatenate(pis), "v": np.concatenate(vs),
            "drawn": o + REF_CHUNK}


_BF16_REF = {}


def bf16_reference(pool, channels):
    if channels not in _BF16_REF:
        params = exact_params(channels, L.EXACT_SEED, L.HEAD_SHIFT[channels])
        folded = L.fold_like_engine(params, channels)
        table = L.conv1_table_ref(folded)
        first = []

        def evaluate(st):
            ref = L.forward_layers(st, folded, dtype=torch.float32, conv1=L.conv1_from_table(st, table))
            rpi, rv, _ = L.heads_ref(ref["fc2"][2], folded)
            if not first:                       # conv1 from its table is conv1_ref, and the f32 evaluation is the float64 one
                first.append(L.forward_layers(st[:8], folded))
                assert first[0]["S1"] <= ref["S1"] and np.array_equal(first[0]["t1"], ref["t1"][:8])
                assert all(np.array_equal(first[0][k][0], ref[k][0][:8]) and np.array_equal(first[0][k][1], ref[k][1][:8]) for k in L.LAYERS)
            keep = bf16_rows_ok(ref, rpi, rv)
            sub = {"S1": ref["S1"], "t1": ref["t1"][keep], **{k: tuple(a[keep] for a in ref[k]) for k in L.LAYERS}}
            L.exact_conditions(sub, rpi[keep], rv[keep])
            return keep, {k: L.bf16_bits(ref[k][2]) for k in L.LAYERS}, rpi, rv

        _BF16_REF[channels] = dict(build_reference(pool, evaluate, L.LAYERS), params=params)
    return _BF16_REF[channels]


_FP8_REF = {}


def fp8_reference(pool, channels, sa2, sa3):
    key = (channels, sa2, sa3)
    if key not in _FP8_REF:
        params = exact_params(channels, L.EXACT_SEED, L8.HEAD_SHIFT[channels])
        table = L.conv1_table_ref(L.fold_like_engine(params, channels))
        first = []

        def evaluate(st):
            ref = L8.forward_exact(st, params, channels, sa2, sa3, conv1=L.conv1_from_table(st, table))
            if not first:
                first.append(L8.forward_exact(st[:8], params, channels, sa2, sa3, dtype=torch.float64))
                assert all(np.array_equal(first[0][k], ref[k][:8]) for k in FP8_LAYERS)
            keep = fp8_rows_ok(ref)
            sub = dict(ref, conv2=tuple(a[keep] for a in ref["conv2"]), pi=ref["pi"][keep], v=ref["v"][keep],
                       **{k + "_yS": tuple(a[keep] for a in ref[k + "_yS"]) for k in ("fc1", "fc2")}, **{k: ref[k][keep] for k in FP8_LAYERS})
            L8.exact_conditions(sub)            # (its "units" and "scaled_max" are maxima over the chunk: asserted for every row drawn)
            return keep, {k: ref[k] for k in FP8_LAYERS}, ref["pi"], ref["v"]

        _FP8_REF[key] = dict(build_reference(pool, evaluate, tuple(FP8_LAYERS)), params=params)
    return _FP8_REF[key]


# ---- one diagnostic engine per width and class, its reader, its chunked (pi, v) -------------------------------------------
class Rig:
    def __init__(self, engine_mod, channels, cls):
        self.channels, self.cls = channels, cls
        self.e = engine_mod.Engine(device=0, max_batch=MB, net_channels=channels, diag=True)
        self.reader = Reader(channels, FP8_LAYERS if cls == "fp8" else BF16_LAYERS)
        self.fp8_class = engine_mod.NET_CLASS_FP8
        self.loaded = {}

    def load(self, model_id, params, states, with_layers=False):
        """Upload, pin the class, and forward `states` through predict_states in chunks of 128, once per model."""
        if model_id not in self.loaded:
            self.e.net_set_params(model_id, params)
            if self.cls == "fp8":
                self.e.net_set_class(model_id, self.fp8_class)
            set_options(self.e, {})
            self.loaded[model_id] = chunked_predict(self.e, model_id, states, self.reader if with_layers else None)
        return self.loaded[model_id]


@pytest.fixture(scope="module")
def rigs(engine_mod):
    made = {}

    def get(channels, cls):
        if (channels, cls) not in made:
            made[(channels, cls)] = Rig(engine_mod, channels, cls)
        return made[(channels, cls)]

    yield get
    for rig in made.values():
        rig.e.close()


# ---- the entry itself -------------------------------------------------------------------------------------------------
def test_hinted_forward_refuses_and_fills(engine_mod, rigs, pool):
    """az_diag_predict_hinted: -1 and nothing written for n < 1, rows_hint < n or > max_batch, rows_typ < 0, an unknown or non-conv
    model, "eval_mirror" on; otherwise rows [0, n) are predict_states' rows and rows [n, rows_hint) the sentinel.  The shipped
    library does not export it."""
    rig = rigs(256, "bf16")
    e = rig.e
    e.net_init_random(7, seed=3)
    e.net_set_kind(8, engine_mod.NET_HASH, 5)
    st = pool[:40]
    for model, n, hint, typ in ((7, 0, 8, 0), (7, 9, 8, 0), (7, 8, MB + 1, 0), (7, 8, 8, -1), (9, 8, 8, 0), (8, 8, 8, 0)):
        assert hinted(e, model, st[:n], hint, typ) is None, (model, n, hint, typ)
    e.set_option("eval_mirror", 1)
    try:
        assert hinted(e, 7, st[:8], 8, 0) is None
    finally:
        e.set_option("eval_mirror", 0)
    want = e.predict_states(st, 7)
    for hint, typ in ((40, 0), (64, 64), (MB, 0), (MB, 100), (MB, 2 * MB)):
        pi, v = hinted(e, 7, st, hint, typ)
        assert np.array_equal(pi[:40], want[0]) and np.array_equal(v[:40], want[1]), (hint, typ)
        assert (pi[40:].view(np.uint32) == SENTINEL).all() and (v[40:].view(np.uint32) == SENTINEL).all(), (hint, typ)
    assert not hasattr(engine_mod._lib, "az_diag_predict_hinted")


# ---- exact data -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "shipped" if not o else ",".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("channels", [512, 256])
def test_exact_data_every_route_bit_for_bit(rigs, pool, channels, opts):
    ref = bf16_reference(pool, channels)                               # its conditions are asserted before the device is touched
    rig = rigs(channels, "bf16")
    pi0, v0, _ = rig.load(0, ref["params"], ref["states"])
    assert np.abs(pi0 - ref["pi"]).max() <= 1e-6 and np.abs(v0 - ref["v"]).max() <= 1e-6
    try:
        set_options(rig.e, opts)
        sweep(rig.e, 0, channels, f"bf16 exact data {opts}", triples(channels, "bf16"), ref["states"], ref["layers"], pi0, v0, rig.reader,
              ref_heads=(ref["pi"], ref["v"]))
    finally:
        set_options(rig.e, {})


@pytest.mark.parametrize("opts", FP8_OPTION_SETS, ids=lambda o: "shipped" if not o else ",".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("channels", [512, 256])
def test_exact_data_every_route_bit_for_bit_fp8(rigs, pool, channels, opts):
    rig = rigs(channels, "fp8")
    params = exact_params(channels, L.EXACT_SEED, L8.HEAD_SHIFT[channels])
    if 0 not in rig.loaded:                                            # the scales are the engine's own: the upload comes first
        rig.e.net_set_params(0, params)
        rig.e.net_set_class(0, rig.fp8_class)
    sa2, sa3 = fp8_scales(rig.e, 0)
    ref = fp8_reference(pool, channels, sa2, sa3)
    pi0, v0, _ = rig.load(0, ref["params"], ref["states"])
    assert np.abs(pi0 - ref["pi"]).max() <= 1e-6 and np.abs(v0 - ref["v"]).max() <= 1e-6
    try:
        set_options(rig.e, opts)
        sweep(rig.e, 0, channels, f"fp8 exact data {opts}", triples(channels, "fp8"), ref["states"], ref["layers"], pi0, v0, rig.reader,
              ref_heads=(ref["pi"], ref["v"]), fp8_narrow=opts.get("narrow_rows", DEFAULTS["narrow_rows"]))
    finally:
        set_options(rig.e, {})


# ---- random data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["bf16", "fp8"])
@pytest.mark.parametrize("channels", [512, 256])
def test_random_data_every_route_is_the_chunked_forward(rigs, pool, channels, cls):
    """random_params, the shipped options: every hinted forward's layers and (pi, v) are, bit for bit, those of the same states
    through predict_states in chunks of 128 (read chunk by chunk, once)."""
    rig = rigs(channels, cls)
    states = pool[MB:]                                                 # the pool's other half: no exact-data condition is needed here
    pi0, v0, layers = rig.load(1, random_params(channels, seed=40 + channels), states, with_layers=True)
    assert np.isfinite(pi0).all() and np.isfinite(v0).all() and all(bool(t.any()) for t in layers.values())
    sweep(rig.e, 1, channels, f"{cls} random data", triples(channels, cls), states, layers, pi0, v0, rig.reader,
          fp8_narrow=DEFAULTS["narrow_rows"] if cls == "fp8" else None)
