"""The C entries of the PISGradNet shell (include/dpi.h: dpi_fit_shell_workspace_bytes, dpi_fit_shell_forward,
dpi_fit_shell_loss, dpi_fit_shell_backward) on a host without a GPU: additions within ABI 8; every refusal returns
its code and names its cap before any device work.  CPU only."""
import ctypes

import pytest

from deeppicarditeration_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from deeppicarditeration_amd.build import build
    build(verbose=False)
    return _lib.load()


PTR = ctypes.c_void_p(4096)


def _tab(depth, hole=None):
    n = 5 + 2 * (depth + 2)
    return (ctypes.c_void_p * n)(*[None if k == hole else 4096 for k in range(n)])


def _fwd(lib, nx=10, depth=2, B=4, tables=True, hole=None, ws=PTR, ws_bytes=None, tx_stride=None, problem=None, **null):
    """dpi_fit_shell_forward with non-null dummy device pointers (never dereferenced on a refusal)."""
    if ws_bytes is None:
        ws_bytes = lib.dpi_fit_shell_workspace_bytes(nx, depth, B)
    p = {k: null.get(k, PTR) for k in ("coeff", "tx", "tau", "s", "res", "res_x")}
    return lib.dpi_fit_shell_forward(problem, 1.0, nx, depth, p["coeff"], _tab(depth, hole) if tables else None, p["tx"],
                                     1 + nx if tx_stride is None else tx_stride, B, 1, p["tau"], p["s"], p["res"],
                                     p["res_x"], ws, ws_bytes, None)


def _loss(lib, nx=10, depth=2, B=4, ws=PTR, ws_bytes=None, kind=0, clip=0.0, kappa=1.0, y_stride=None, **null):
    if ws_bytes is None:
        ws_bytes = lib.dpi_fit_shell_workspace_bytes(nx, depth, B)
    p = {k: null.get(k, PTR) for k in ("sp", "q", "s", "res", "res_x", "tx", "y", "losses", "e", "r", "sbar")}
    return lib.dpi_fit_shell_loss(nx, p["sp"], p["q"], p["s"], p["res"], p["res_x"], p["tx"], 1 + nx, p["y"],
                                  1 + nx if y_stride is None else y_stride, B, 0.0, kind, clip, kappa, p["losses"],
                                  p["e"], p["r"], p["sbar"], ws, ws_bytes, None)


def _bwd(lib, nx=10, depth=2, B=4, tables=True, hole=None, grad_tables=True, grad_hole=None, ws=PTR, ws_bytes=None,
         dtau=PTR, sbar=PTR):
    if ws_bytes is None:
        ws_bytes = lib.dpi_fit_shell_workspace_bytes(nx, depth, B)
    return lib.dpi_fit_shell_backward(nx, depth, _tab(depth, hole) if tables else None,
                                      _tab(depth, grad_hole) if grad_tables else None, dtau, sbar, B, ws, ws_bytes, None)


def test_symbols_are_additions_within_abi_8(lib):
    assert lib.dpi_abi_version() == 8 and _lib.DPI_ABI_VERSION == 8
    S = _lib.SIGNATURES
    c_int, c_void_p, c_size_t, c_float, c_double, TAB = (ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float,
                                                         ctypes.c_double, ctypes.POINTER(ctypes.c_void_p))
    assert S["dpi_fit_shell_workspace_bytes"] == (c_size_t, [c_int, c_int, c_int])
    assert S["dpi_fit_shell_forward"] == (c_int, [c_void_p, c_double, c_int, c_int, c_void_p, TAB, c_void_p, c_int,
                                                  c_int, c_int] + [c_void_p] * 5 + [c_size_t, c_void_p])
    assert S["dpi_fit_shell_loss"] == (c_int, [c_int] + [c_void_p] * 6 + [c_int, c_void_p, c_int, c_int, c_float, c_int,
                                               c_float, c_float] + [c_void_p] * 5 + [c_size_t, c_void_p])
    assert S["dpi_fit_shell_backward"] == (c_int, [c_int, c_int, TAB, TAB, c_void_p, c_void_p, c_int, c_void_p, c_size_t,
                                                   c_void_p])
    for name in ("workspace_bytes", "forward", "loss", "backward"):
        fn = getattr(lib, f"dpi_fit_shell_{name}")
        assert (fn.restype, list(fn.argtypes)) == S[f"dpi_fit_shell_{name}"]
    # every earlier entry is still there
    assert {"dpi_fit_core_forward", "dpi_fit_core_layers_backward", "dpi_fit_gradients", "dpi_fit_step"} <= set(S)


@pytest.mark.parametrize("call", [_fwd, _loss, _bwd], ids=["forward", "loss", "backward"])
def test_caps_are_named_before_device_work(lib, call):
    assert call(lib, nx=129, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED and "nx = 129 > 128" in _lib.last_error()
    assert call(lib, nx=0, ws_bytes=0) == _lib.DPI_ERR_ARG
    assert call(lib, B=0, ws_bytes=1 << 30) == _lib.DPI_ERR_ARG and "B = 0 < 1" in _lib.last_error()
    assert call(lib, B=-1, ws_bytes=0) == _lib.DPI_ERR_ARG
    assert call(lib, B=(1 << 24) + 1, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED and "2^24" in _lib.last_error()
    need = lib.dpi_fit_shell_workspace_bytes(10, 2, 4)
    assert need > 0
    assert call(lib, ws_bytes=7) == _lib.DPI_ERR_WORKSPACE
    assert "workspace too small" in _lib.last_error() and "dpi_fit_shell_workspace_bytes" in _lib.last_error()
    assert call(lib, ws=None) == _lib.DPI_ERR_WORKSPACE
    assert call(lib, ws=ctypes.c_void_p(4100)) == _lib.DPI_ERR_ARG and "8-byte aligned" in _lib.last_error()
    assert "fit_shell_" in _lib.last_error()


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_depth_tables_and_workspace(lib, call):
    assert call(lib, depth=5, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED
    assert "smooth_net depth 5 > 4" in _lib.last_error()
    assert call(lib, depth=0, ws_bytes=0) == _lib.DPI_ERR_ARG
    assert call(lib, tables=False) == _lib.DPI_ERR_ARG and "null pointer table" in _lib.last_error()
    for hole in (0, 4, 12):
        assert call(lib, hole=hole) == _lib.DPI_ERR_ARG and f"null entry {hole} in the parameter table" in _lib.last_error()
    need = lib.dpi_fit_shell_workspace_bytes(10, 2, 4)
    assert call(lib, ws_bytes=need - 1) == _lib.DPI_ERR_WORKSPACE
    assert f"{need - 1} < {need} bytes" in _lib.last_error()


def test_forward_pointers_problem_and_strides(lib):
    assert _fwd(lib, tx_stride=10) == _lib.DPI_ERR_ARG and "stride" in _lib.last_error()
    for null in ("coeff", "tx", "tau", "s", "res", "res_x"):
        assert _fwd(lib, **{null: None}) == _lib.DPI_ERR_ARG and "null coeff, tx, tau" in _lib.last_error()
    # exactly enough workspace passes the workspace check: the null problem is the next refusal
    assert _fwd(lib) == _lib.DPI_ERR_ARG and "null problem" in _lib.last_error()
    assert _fwd(lib, depth=4, nx=128, B=512) == _lib.DPI_ERR_ARG and "null problem" in _lib.last_error()  # the caps pass


def test_loss_and_backward_pointers(lib):
    assert _loss(lib, y_stride=10) == _lib.DPI_ERR_ARG and "stride" in _lib.last_error()
    assert _loss(lib, kind=2) == _lib.DPI_ERR_ARG and "loss kind" in _lib.last_error()
    assert _loss(lib, kind=1, clip=0.0) == _lib.DPI_ERR_ARG and "clip" in _lib.last_error()
    assert _loss(lib, kappa=-1.0) == _lib.DPI_ERR_ARG and "kappa" in _lib.last_error()
    for null in ("sp", "s", "res", "tx", "y", "losses", "e", "sbar"):
        assert _loss(lib, **{null: None}) == _lib.DPI_ERR_ARG and "null sp, s, res" in _lib.last_error()
    for null in ("res_x", "r"):
        assert _loss(lib, **{null: None}) == _lib.DPI_ERR_ARG and "null res_x or r" in _lib.last_error()
    need = 8 * 1 * 11  # its own region: the tiles' sums
    assert _loss(lib, ws_bytes=need - 1) == _lib.DPI_ERR_WORKSPACE and f"< {need} bytes" in _lib.last_error()
    assert _bwd(lib, grad_tables=False) == _lib.DPI_ERR_ARG and "null pointer table (grads)" in _lib.last_error()
    assert _bwd(lib, grad_hole=3) == _lib.DPI_ERR_ARG and "null entry 3 in the gradient table" in _lib.last_error()
    assert _bwd(lib, dtau=None) == _lib.DPI_ERR_ARG and "null dtau or sbar" in _lib.last_error()
    assert _bwd(lib, sbar=None) == _lib.DPI_ERR_ARG and "null dtau or sbar" in _lib.last_error()


def test_workspace_steps_by_tiles_and_refused_shapes_have_none(lib):
    sizes = [lib.dpi_fit_shell_workspace_bytes(100, 4, B) for B in (1, 64, 65, 100, 128, 512)]
    assert sizes == sorted(sizes) and all(s > 0 and s % 8 == 0 for s in sizes)
    assert sizes[0] == sizes[1] < sizes[2] == sizes[3] == sizes[4] < sizes[5]
    assert lib.dpi_fit_shell_workspace_bytes(100, 1, 64) < lib.dpi_fit_shell_workspace_bytes(100, 4, 64)
    for nx, depth, B in ((129, 1, 64), (0, 1, 64), (10, 5, 64), (10, 0, 64), (10, 1, 0), (10, 1, -1)):
        assert lib.dpi_fit_shell_workspace_bytes(nx, depth, B) == 0
