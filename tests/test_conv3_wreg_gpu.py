"""conv3 with its weight operand in a register ring (k_conv3_auto_wreg, "conv3_wreg" = 1) against the same tile with the weight
tile in LDS (k_conv3_auto, "conv3_wreg" = 0): the K order per accumulator is the same, so conv3's output and the whole forward
must be the same BITS, at row counts on either side of every device-side line (hand-over to the small-batch kernels, half-tile
tail on / off, one / two rounds of workgroups, a full batch), with and without the half-tile tail, and again after a second
weight upload into the same model id (the fragment-ordered copy of the weights follows the weights).  Every row is compared."""
import ctypes as C

import numpy as np
import pytest

from test_net_gpu import random_states

pytestmark = pytest.mark.gpu
CH = 512
ROWS = (1, 12, 13, 128, 356, 357, 768, 1536, 1537, 2300, 3100, 8192)


def _conv3_out(e, rows):
    """conv3's output of the engine's last forward: rows x [4][5][CH] bf16 as uint16 (diagnostic library's reader)."""
    f = e._lib.az_diag_read_conv3_out
    f.restype = C.c_longlong
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    out = np.empty((rows, 20, CH), np.uint16)
    assert f(e._h, rows, out.ctypes.data_as(C.c_void_p)) == out.nbytes
    return out


def _check_model(diag, shipped, states, model_id, tag):
    for small in (1, 0):            # the shipped hand-over to the small-batch kernels / the image-resident kernel at every row count
        for e in (diag, shipped):
            e.set_option("conv3_small", small)
            e.set_option("narrow_rows", 32 if small else 0)
        for tail in (1, 0):
            for e in (diag, shipped):
                e.set_option("conv3_tail", tail)
            for n in ROWS:
                diag.set_option("conv3_wreg", 0)
                ref = diag.predict_states(states[:n], model_id)
                ref3 = _conv3_out(diag, n)
                diag.set_option("conv3_wreg", 1)
                got = diag.predict_states(states[:n], model_id)
                got3 = _conv3_out(diag, n)
                where = (tag, small, tail, n)
                assert np.isfinite(ref[0]).all() and ref3.any(), where
                assert np.array_equal(got3, ref3), (where, "conv3 rows that differ", np.unique(np.nonzero(got3 != ref3)[0])[:8])
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), where
                shipped.set_option("conv3_wreg", 0)
                sref = shipped.predict_states(states[:n], model_id)
                shipped.set_option("conv3_wreg", 1)
                sgot = shipped.predict_states(states[:n], model_id)
                assert np.array_equal(sgot[0], sref[0]) and np.array_equal(sgot[1], sref[1]), where
                assert np.array_equal(sgot[0], ref[0]) and np.array_equal(sgot[1], ref[1]), where     # and the two libraries agree


def test_conv3_weights_from_registers_are_bit_identical(engine, engine_mod, oracle):
    states = random_states(oracle, 8192, seed=321)
    diag = engine_mod.Engine(device=0, max_batch=8192, net_channels=CH, diag=True)
    keys = (("conv3_wreg", 1), ("conv3_tail", 1), ("conv3_small", 1), ("narrow_rows", 32))
    try:
        engine.net_init_random(27, seed=41)
        diag.net_set_params(27, engine.net_get_params(27))
        _check_model(diag, engine, states, 27, "first upload")
        # a second upload into the same model id: other weights, and the fragment-ordered copy must be theirs
        before = engine.predict_states(states[:357], 27)
        engine.net_init_random(27, seed=42)
        diag.net_set_params(27, engine.net_get_params(27))
        after = engine.predict_states(states[:357], 27)
        assert not np.array_equal(before[0], after[0])
        _check_model(diag, engine, states, 27, "second upload")
    finally:
        for k, v in keys:
            engine.set_option(k, v)
        engine.net_free(27)
        diag.close()
