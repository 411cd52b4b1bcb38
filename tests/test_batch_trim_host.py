"""CPU: trimmed pairs in fgoicp_batch without a GPU — fgoicp_batch_create's per-pair trim fractions (fgoicp_batch_opts.trim_fractions)
and the refusals of the test hook fgoicp_batch_test_trim_bounds, which all come before any device work."""
import ctypes as C

import numpy as np


def _opts(fg, trim=None, solver_trim=0.0, struct_size=None):
    L = fg._lib
    o = L.BatchOpts(C.sizeof(L.BatchOpts), L.SolverOpts(0, 1, 0, 0, float(solver_trim)), 0, None)
    if trim is not None:
        o.trim_fractions = trim.ctypes.data_as(L.c_float_p)
    if struct_size is not None:
        o.struct_size = struct_size
    return o


def _create(fg, n, opts):
    lib = fg._lib.load()
    pts = np.random.default_rng(0).uniform(-1, 1, (64, 3)).astype(np.float32)
    fp = pts.ctypes.data_as(fg._lib.c_float_p)
    arr = (fg._lib.BatchPair * n)(*[fg._lib.BatchPair(fp, 64, fp, 64, 0.05, 1e-3) for _ in range(n)])
    h = C.c_void_p()
    rc = lib.fgoicp_batch_create(arr, n, C.byref(opts), C.byref(h))
    if h.value:
        lib.fgoicp_batch_destroy(h)
    return rc


def test_create_takes_per_pair_trim_fractions(fg):
    trim = np.array([0.0, 0.1, 0.25], np.float32)
    assert _create(fg, 3, _opts(fg, trim)) == 0
    assert _create(fg, 3, _opts(fg)) == 0  # NULL: no pair trimmed
    assert _create(fg, 1, _opts(fg, np.array([0.999], np.float32))) == 0


def test_create_refuses_bad_trim_fractions(fg):
    for bad in (np.nan, -0.1, 1.0, 1.5, np.inf):
        trim = np.array([0.0, bad, 0.1], np.float32)
        assert _create(fg, 3, _opts(fg, trim)) == 1, bad
        assert b"trim_fractions[1]" in fg._lib.load().fgoicp_last_error()
    # the batch-wide fraction keeps its refusal, with or without per-pair fractions
    assert _create(fg, 1, _opts(fg, solver_trim=0.1)) == 1
    assert _create(fg, 1, _opts(fg, np.array([0.1], np.float32), solver_trim=0.1)) == 1


def test_struct_ending_at_max_live_has_no_trim_fractions(fg):
    """a caller compiled before trim_fractions existed: its struct ends at max_live, and whatever lies behind it is not read"""
    L = fg._lib
    end = L.BatchOpts.trim_fractions.offset
    nan = np.array([np.nan], np.float32)  # refused if it were read
    assert _create(fg, 1, _opts(fg, nan)) == 1
    assert _create(fg, 1, _opts(fg, nan, struct_size=end)) == 0


def test_python_batch_takes_trim_fractions(fg):
    """FastGoICPBatch(trim_fraction=...) as every pair's default, a fifth tuple member per pair; a bad one is refused at create"""
    import pytest
    pts = np.random.default_rng(1).uniform(-1, 1, (50, 3)).astype(np.float32)
    b = fg.FastGoICPBatch([(pts, pts), (pts, pts, 0.05, 1e-3, 0.25)], trim_fraction=0.1)
    b.close()
    with pytest.raises(fg.FgoicpError):
        fg.FastGoICPBatch([(pts, pts, 0.05, 1e-3, 1.0)])
    with pytest.raises(fg.FgoicpError):
        fg.FastGoICPBatch([(pts, pts)], trim_fraction=-0.5)


def test_trim_bounds_hook_refuses_before_device_work(fg):
    lib = fg._lib.load()
    one, zero = (C.c_int * 2)(1, 1), (C.c_int * 2)(0, 0)
    offs = (C.c_int * 2)(0, 1)
    fake = (C.c_void_p * 2)(None, None)
    buf = np.zeros(18, np.float32)
    b = buf.ctypes.data_as(fg._lib.c_float_p)
    n_out, s_out = C.c_uint64(7), C.c_uint64(9)
    tb = lib.fgoicp_batch_test_trim_bounds
    assert tb(None, 1, 1, zero, one, b, b, zero, offs, b, b, b, C.byref(n_out), 0, C.byref(s_out)) == 1
    assert tb(fake, 0, 0, None, None, None, None, None, None, None, None, None, None, 0, None) == 1  # no contexts
    assert tb(fake, 1, -1, None, None, None, None, None, None, None, None, None, None, 0, None) == 1  # nreq < 0
    assert tb(fake, 1, 1, None, one, b, b, zero, offs, b, b, b, None, 0, None) == 1
    assert tb(fake, 1, 1, zero, None, b, b, zero, offs, b, b, b, None, 0, None) == 1
    assert tb(fake, 1, 1, zero, one, b, b, zero, None, b, b, b, None, 0, None) == 1
    assert tb(fake, 1, 1, zero, one, b, b, zero, offs, b, b, b, C.byref(n_out), 3, C.byref(s_out)) == 1  # a null context
    assert b"fgoicp_batch_test_trim_bounds" in lib.fgoicp_last_error()
    assert (n_out.value, s_out.value) == (7, 9)  # nothing written on refusal
