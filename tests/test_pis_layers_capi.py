"""The C entries of the layer-wise PISGradNet core (include/dpi.h: dpi_fit_core_layers_workspace_bytes,
dpi_fit_core_layers_forward, dpi_fit_core_layers_backward) on a host without a GPU: additions within ABI 8 with
the contract of dpi_fit_core_*; every refusal returns its code and names its reason before any device work.
CPU only."""
import ctypes

import pytest

from deeppicarditeration_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from deeppicarditeration_amd.build import build
    build(verbose=False)
    return _lib.load()


def _w(widths):
    return (ctypes.c_int * max(len(widths), 1))(*widths)


def _tab(n, hole=None):
    return (ctypes.c_void_p * n)(*[None if k == hole else 4096 for k in range(n)])


PTR = ctypes.c_void_p(4096)


def _fwd(lib, nx=10, widths=(16, 16), tables=True, B=4, ws_bytes=None, tau_stride=64, x_stride=None, tau=PTR, x=PTR,
         sp=PTR, q=PTR, ws=PTR, hole=None):
    """dpi_fit_core_layers_forward with non-null dummy device pointers (never dereferenced on a refusal)."""
    L = len(widths)
    if ws_bytes is None:
        ws_bytes = lib.dpi_fit_core_layers_workspace_bytes(nx, L, _w(widths), B)
    tab = _tab(L + 1, hole) if tables else None
    return lib.dpi_fit_core_layers_forward(nx, L, _w(widths), tab, tab, tau, tau_stride, x,
                                           nx if x_stride is None else x_stride, B, sp, q, ws, ws_bytes, None)


def _bwd(lib, nx=10, widths=(16, 16), tables=True, B=4, ws_bytes=None, e=PTR, r=PTR, dtau=PTR, ws=PTR, hole=None,
         grad_hole=None, grad_tables=True):
    L = len(widths)
    if ws_bytes is None:
        ws_bytes = lib.dpi_fit_core_layers_workspace_bytes(nx, L, _w(widths), B)
    tab = _tab(L + 1, hole) if tables else None
    gtab = _tab(L + 1, grad_hole) if grad_tables else None
    return lib.dpi_fit_core_layers_backward(nx, L, _w(widths), tab, tab, gtab, gtab, e, r, B, dtau, ws, ws_bytes, None)


def test_symbols_are_additions_within_abi_8(lib):
    assert lib.dpi_abi_version() == 8 and _lib.DPI_ABI_VERSION == 8
    new = {"dpi_fit_core_layers_workspace_bytes", "dpi_fit_core_layers_forward", "dpi_fit_core_layers_backward"}
    assert new <= set(_lib.SIGNATURES)
    assert lib.dpi_fit_core_layers_workspace_bytes.restype is ctypes.c_size_t
    for form in ("", "_layers"):  # same arguments as the entries they stand beside
        for entry in ("workspace_bytes", "forward", "backward"):
            assert _lib.SIGNATURES[f"dpi_fit_core{form}_{entry}"] == _lib.SIGNATURES[f"dpi_fit_core_{entry}"]


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_caps_are_named_before_device_work(lib, call):
    assert call(lib, widths=(16, 513), ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED
    assert "513 > 512" in _lib.last_error()
    assert call(lib, widths=(8,) * 5, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED
    assert "5 hidden layers > 4" in _lib.last_error()
    assert call(lib, nx=129, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED and "nx = 129 > 128" in _lib.last_error()
    assert call(lib, B=(1 << 24) + 1, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED and "2^24" in _lib.last_error()
    assert call(lib, nx=0, ws_bytes=0) == _lib.DPI_ERR_ARG
    assert call(lib, widths=(), ws_bytes=0) == _lib.DPI_ERR_ARG
    assert call(lib, B=-1, ws_bytes=0) == _lib.DPI_ERR_ARG
    assert call(lib, widths=(16, 0), ws_bytes=0) == _lib.DPI_ERR_ARG and "width < 1" in _lib.last_error()
    assert call(lib, tables=False) == _lib.DPI_ERR_ARG and "null pointer table" in _lib.last_error()
    for hole in (0, 1, 2):
        assert call(lib, hole=hole) == _lib.DPI_ERR_ARG and f"layer {hole}" in _lib.last_error()
    need = lib.dpi_fit_core_layers_workspace_bytes(10, 2, _w((16, 16)), 4)
    assert need > 0
    assert call(lib, ws_bytes=need - 1) == _lib.DPI_ERR_WORKSPACE
    assert "workspace too small" in _lib.last_error() and "dpi_fit_core_layers_workspace_bytes" in _lib.last_error()
    assert call(lib, ws=None) == _lib.DPI_ERR_WORKSPACE
    assert call(lib, ws=ctypes.c_void_p(4098)) == _lib.DPI_ERR_ARG and "4-byte aligned" in _lib.last_error()
    assert call(lib, widths=(512,) * 4, nx=128, ws_bytes=0) == _lib.DPI_ERR_WORKSPACE  # the caps themselves pass
    assert "fit_core_layers_" in _lib.last_error()


def test_pointers_and_strides(lib):
    assert _fwd(lib, tau_stride=63) == _lib.DPI_ERR_ARG and "stride" in _lib.last_error()
    assert _fwd(lib, x_stride=9) == _lib.DPI_ERR_ARG and "stride" in _lib.last_error()
    for null in ("tau", "x", "sp"):
        assert _fwd(lib, **{null: None}) == _lib.DPI_ERR_ARG and "null tau, x or sp" in _lib.last_error()
    assert _bwd(lib, e=None) == _lib.DPI_ERR_ARG and "null e" in _lib.last_error()
    assert _bwd(lib, dtau=None) == _lib.DPI_ERR_ARG and "null e or dtau" in _lib.last_error()
    assert _bwd(lib, grad_tables=False) == _lib.DPI_ERR_ARG and "null pointer table (dW, db)" in _lib.last_error()
    assert _bwd(lib, grad_hole=2) == _lib.DPI_ERR_ARG and "gradient table at layer 2" in _lib.last_error()


def test_empty_batch_launches_nothing(lib):
    w = _w((16, 16))
    assert lib.dpi_fit_core_layers_forward(10, 2, w, None, None, None, 64, None, 10, 0, None, None, None, 0,
                                           None) == _lib.DPI_OK
    assert lib.dpi_fit_core_layers_backward(10, 2, w, None, None, None, None, None, None, 0, None, None, 0,
                                            None) == _lib.DPI_OK
    # the scalar arguments are still checked
    assert lib.dpi_fit_core_layers_forward(10, 2, w, None, None, None, 63, None, 10, 0, None, None, None, 0,
                                           None) == _lib.DPI_ERR_ARG
    assert lib.dpi_fit_core_layers_backward(129, 2, w, None, None, None, None, None, None, 0, None, None, 0,
                                            None) == _lib.DPI_ERR_UNSUPPORTED


SHAPES = [(1, (1,)), (3, (16,)), (10, (64,) * 4), (2, (15, 33)), (5, (48, 16, 31)), (127, (17, 511)), (128, (512,) * 4)]


@pytest.mark.parametrize("nx, widths", SHAPES)
def test_workspace_is_positive_for_every_accepted_shape_and_covers_the_tiles_form(lib, nx, widths):
    L, w = len(widths), _w(widths)
    for B in (1, 17, 64, 65, 512):
        need = lib.dpi_fit_core_layers_workspace_bytes(nx, L, w, B)
        assert need > 0 and need % 4 == 0
        assert need >= lib.dpi_fit_core_workspace_bytes(nx, L, w, B)
        # exactly enough passes the workspace check (a null tau is the next refusal), one byte less does not
        assert _fwd(lib, nx=nx, widths=widths, B=B, ws_bytes=need, tau=None) == _lib.DPI_ERR_ARG
        assert "null tau" in _lib.last_error()
        assert _fwd(lib, nx=nx, widths=widths, B=B, ws_bytes=need - 1) == _lib.DPI_ERR_WORKSPACE
        assert _bwd(lib, nx=nx, widths=widths, B=B, ws_bytes=need - 1) == _lib.DPI_ERR_WORKSPACE


def test_workspace_steps_by_tiles_and_refused_shapes_have_none(lib):
    w = _w((512,) * 4)
    sizes = [lib.dpi_fit_core_layers_workspace_bytes(100, 4, w, B) for B in (0, 1, 64, 65, 100, 128, 512)]
    assert sizes == sorted(sizes) and sizes[0] == 0
    assert sizes[1] == sizes[2] < sizes[3] == sizes[4] == sizes[5] < sizes[6]
    assert lib.dpi_fit_core_layers_workspace_bytes(100, 5, _w((8,) * 5), 64) == 0
    assert lib.dpi_fit_core_layers_workspace_bytes(129, 1, _w((8,)), 64) == 0
    assert lib.dpi_fit_core_layers_workspace_bytes(10, 1, _w((513,)), 64) == 0
    assert lib.dpi_fit_core_layers_workspace_bytes(10, 1, _w((0,)), 64) == 0
    assert lib.dpi_fit_core_layers_workspace_bytes(10, 0, _w(()), 64) == 0
    assert lib.dpi_fit_core_layers_workspace_bytes(10, 1, None, 64) == 0
    assert lib.dpi_fit_core_layers_workspace_bytes(10, 1, _w((8,)), -1) == 0
