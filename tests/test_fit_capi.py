"""The fit entry points of the C ABI (include/dpi.h: dpi_fit_workspace_bytes, dpi_fit_gradients) on a
host without a GPU: both are additions within ABI 8, every refusal returns its code and names its reason
before any device work, and an empty batch launches nothing."""
import ctypes

import pytest

from deeppicarditeration_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from deeppicarditeration_amd.build import build
    build(verbose=False)
    return _lib.load()


def _call(lib, n_in=8, widths=(16, 16), act=_lib.DPI_ACT_ELU, tables=True, B=4, loss=_lib.DPI_FIT_LOSS_SQUARE,
          clip=0.0, c=1.0, ws_bytes=None, y_stride=None, n_hidden=None):
    """dpi_fit_gradients with non-null dummy device pointers (never dereferenced on a refusal)."""
    n_hidden = len(widths) if n_hidden is None else n_hidden
    w = (ctypes.c_int * max(len(widths), 1))(*widths)
    ptr = ctypes.c_void_p(4096)
    tab = (ctypes.c_void_p * (n_hidden + 1))(*[4096] * (n_hidden + 1)) if tables else None
    if ws_bytes is None:
        ws_bytes = lib.dpi_fit_workspace_bytes(n_in, n_hidden, w, B)
    return lib.dpi_fit_gradients(n_in, n_hidden, w, act, tab, tab, tab, tab, ptr, ptr,
                                 n_in if y_stride is None else y_stride, B, 0.5, loss, clip, c, ptr, ptr, ws_bytes,
                                 None)


def test_symbols_are_additions_within_abi_8(lib):
    assert lib.dpi_abi_version() == 8 and _lib.DPI_ABI_VERSION == 8
    assert {"dpi_fit_workspace_bytes", "dpi_fit_gradients"} <= set(_lib.SIGNATURES)
    assert lib.dpi_fit_workspace_bytes.restype is ctypes.c_size_t


def test_refusals_come_before_device_work(lib):
    assert _call(lib, widths=(16, 257), ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED
    assert "257 > 256" in _lib.last_error()
    assert _call(lib, widths=(8,) * 9, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED
    assert "9 hidden layers" in _lib.last_error()
    assert _call(lib, n_in=258, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED and "nx = 257" in _lib.last_error()
    assert _call(lib, act=3) == _lib.DPI_ERR_UNSUPPORTED and "activation 3" in _lib.last_error()
    assert _call(lib, tables=False) == _lib.DPI_ERR_ARG and "null pointer table" in _lib.last_error()
    assert _call(lib, loss=2) == _lib.DPI_ERR_ARG and "loss kind" in _lib.last_error()
    assert _call(lib, loss=_lib.DPI_FIT_LOSS_CLIP, clip=0.0) == _lib.DPI_ERR_ARG and "clip" in _lib.last_error()
    assert _call(lib, c=-1.0) == _lib.DPI_ERR_ARG
    assert _call(lib, y_stride=7) == _lib.DPI_ERR_ARG and "stride" in _lib.last_error()
    assert _call(lib, B=-1, ws_bytes=0) == _lib.DPI_ERR_ARG
    assert _call(lib, widths=(16, 0), ws_bytes=0) == _lib.DPI_ERR_ARG
    need = lib.dpi_fit_workspace_bytes(8, 2, (ctypes.c_int * 2)(16, 16), 4)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == _lib.DPI_ERR_WORKSPACE and "workspace too small" in _lib.last_error()


def test_null_table_entry_is_named(lib):
    w = (ctypes.c_int * 2)(16, 16)
    ptr = ctypes.c_void_p(4096)
    good = (ctypes.c_void_p * 3)(4096, 4096, 4096)
    bad = (ctypes.c_void_p * 3)(4096, None, 4096)
    rc = lib.dpi_fit_gradients(8, 2, w, _lib.DPI_ACT_TANH, good, good, bad, good, ptr, ptr, 8, 4, 0.0,
                               _lib.DPI_FIT_LOSS_SQUARE, 0.0, 1.0, ptr, ptr, 1 << 30, None)
    assert rc == _lib.DPI_ERR_ARG and "layer 1" in _lib.last_error()


def test_empty_batch_launches_nothing(lib):
    """B = 0: scalar checks only, NULL data pointers and tables accepted."""
    w = (ctypes.c_int * 2)(16, 16)
    assert lib.dpi_fit_gradients(8, 2, w, _lib.DPI_ACT_ELU, None, None, None, None, None, None, 8, 0, 0.0,
                                 _lib.DPI_FIT_LOSS_SQUARE, 0.0, 1.0, None, None, 0, None) == 0
    assert lib.dpi_fit_gradients(8, 2, w, 3, None, None, None, None, None, None, 8, 0, 0.0,
                                 _lib.DPI_FIT_LOSS_SQUARE, 0.0, 1.0, None, None, 0, None) == _lib.DPI_ERR_UNSUPPORTED


def test_workspace_is_monotone_in_B_and_steps_by_tiles(lib):
    w = (ctypes.c_int * 4)(128, 128, 128, 128)
    sizes = [lib.dpi_fit_workspace_bytes(101, 4, w, B) for B in (0, 1, 63, 64, 65, 100, 128, 512, 4096)]
    assert sizes == sorted(sizes) and sizes[0] == 0
    assert sizes[1] == sizes[2] == sizes[3] < sizes[4] == sizes[5] == sizes[6] < sizes[7] < sizes[8]
    # a shape the call refuses has no workspace
    assert lib.dpi_fit_workspace_bytes(101, 9, (ctypes.c_int * 9)(*[8] * 9), 64) == 0
