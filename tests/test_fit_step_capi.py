"""dpi_fit_step (include/dpi.h) on a host without a GPU: an addition within ABI 8, exported and declared; every
argument error returns its code and names its reason before any device work; an empty batch launches
nothing; dpi_fit_workspace_bytes is what it was."""
import ctypes
import re
from pathlib import Path

import pytest

from deeppicarditeration_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from deeppicarditeration_amd.build import build
    build(verbose=False)
    return _lib.load()


def _call(lib, n_in=8, widths=(16, 16), act=_lib.DPI_ACT_ELU, grads=True, moments=True, B=4,
          loss=_lib.DPI_FIT_LOSS_SQUARE, clip=0.0, c=1.0, ws_bytes=None, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
          wd=0.0, decoupled=0, step=1, bad_moment=None):
    """dpi_fit_step with non-null dummy device pointers (never dereferenced on a refusal)."""
    n_hidden = len(widths)
    w = (ctypes.c_int * n_hidden)(*widths)
    ptr = ctypes.c_void_p(4096)
    tab = (ctypes.c_void_p * (n_hidden + 1))(*[4096] * (n_hidden + 1))
    mom = [tab if moments else None] * 4
    if bad_moment is not None:
        mom[bad_moment] = (ctypes.c_void_p * (n_hidden + 1))(4096, None, *[4096] * (n_hidden - 1))
    g = tab if grads else None
    if ws_bytes is None:
        ws_bytes = lib.dpi_fit_workspace_bytes(n_in, n_hidden, w, B)
    return lib.dpi_fit_step(n_in, n_hidden, w, act, tab, tab, g, g, *mom, ptr, ptr, n_in, B, 0.5, loss, clip, c, lr,
                            beta1, beta2, eps, wd, decoupled, step, ptr, ptr, ws_bytes, None)


def test_symbol_is_an_addition_within_abi_8(lib):
    assert lib.dpi_abi_version() == 8 and _lib.DPI_ABI_VERSION == 8
    assert "dpi_fit_step" in _lib.SIGNATURES and lib.dpi_fit_step.restype is ctypes.c_int
    header = (Path(__file__).resolve().parents[1] / "include" / "dpi.h").read_text()
    assert re.search(r"^int dpi_fit_step\(", header, flags=re.M)
    assert re.search(r"^#define DPI_ABI_VERSION 8$", header, flags=re.M)


@pytest.mark.parametrize("kw, named", [
    ({"step": 0}, "step"), ({"step": -3}, "step"),
    ({"beta1": 1.0}, "beta1"), ({"beta1": -0.1}, "beta1"), ({"beta2": 1.0}, "beta2"), ({"beta2": float("nan")}, "beta2"),
    ({"eps": -1e-8}, "eps"), ({"eps": float("inf")}, "eps"),
    ({"lr": -1e-3}, "lr"), ({"lr": float("nan")}, "lr"),
    ({"wd": -0.01}, "weight_decay"), ({"wd": float("inf")}, "weight_decay"),
    ({"moments": False}, "null moment table"), ({"bad_moment": 2}, "moment table at layer 1"),
    ({"loss": 2}, "loss kind"), ({"c": -1.0}, "gradient weight"),
    ({"loss": _lib.DPI_FIT_LOSS_CLIP, "clip": 0.0}, "clip"),
])
def test_argument_errors_come_before_device_work(lib, kw, named):
    assert _call(lib, **kw) == _lib.DPI_ERR_ARG
    assert "fit_step" in _lib.last_error() and named in _lib.last_error()


def test_unsupported_shapes_and_workspace(lib):
    assert _call(lib, act=3) == _lib.DPI_ERR_UNSUPPORTED and "activation 3" in _lib.last_error()
    assert _call(lib, widths=(16, 257), ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED and "257 > 256" in _lib.last_error()
    assert _call(lib, widths=(8,) * 9, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED
    assert _call(lib, n_in=258, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED
    need = lib.dpi_fit_workspace_bytes(8, 2, (ctypes.c_int * 2)(16, 16), 4)
    assert _call(lib, ws_bytes=need - 1) == _lib.DPI_ERR_WORKSPACE and "workspace too small" in _lib.last_error()
    # the gradient tables may be NULL as whole tables (checked up to the workspace), not one of the two
    assert _call(lib, grads=False, ws_bytes=need - 1) == _lib.DPI_ERR_WORKSPACE
    w = (ctypes.c_int * 2)(16, 16)
    ptr = ctypes.c_void_p(4096)
    tab = (ctypes.c_void_p * 3)(4096, 4096, 4096)
    rc = lib.dpi_fit_step(8, 2, w, _lib.DPI_ACT_ELU, tab, tab, tab, None, tab, tab, tab, tab, ptr, ptr, 8, 4, 0.0,
                          _lib.DPI_FIT_LOSS_SQUARE, 0.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1, ptr, ptr, need, None)
    assert rc == _lib.DPI_ERR_ARG and "null pointer table" in _lib.last_error()


def test_empty_batch_launches_nothing(lib):
    w = (ctypes.c_int * 2)(16, 16)
    args = (None,) * 8 + (None, None, 8, 0, 0.0, _lib.DPI_FIT_LOSS_SQUARE, 0.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    assert lib.dpi_fit_step(8, 2, w, _lib.DPI_ACT_TANH, *args, 1, None, None, 0, None) == 0
    assert lib.dpi_fit_step(8, 2, w, _lib.DPI_ACT_TANH, *args, 0, None, None, 0, None) == _lib.DPI_ERR_ARG


def test_workspace_bytes_are_unchanged(lib):
    """The layout of csrc/dpi_fit.hip, restated: five [unit][row] families and the tiles' fp64 partials."""
    def want(n_in, widths, B):
        tiles = (B + 63) // 64
        R = tiles * 64
        h = sum(widths)
        o = (2 * h + 2 * (h + 1) + (n_in + h)) * R
        o += o & 1
        return 4 * (o + 2 * tiles * (n_in + 1))
    for n_in, widths, B in [(8, (16, 16), 4), (101, (128,) * 4, 512), (8, (129,), 65), (257, (256,) * 8, 100)]:
        w = (ctypes.c_int * len(widths))(*widths)
        assert lib.dpi_fit_workspace_bytes(n_in, len(widths), w, B) == want(n_in, widths, B)
