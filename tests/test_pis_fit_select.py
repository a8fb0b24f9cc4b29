"""PISGradNet under TRAIN.BACKEND: hip — what the device objective accepts and refuses, and the C entries
of the core (include/dpi.h: dpi_fit_core_workspace_bytes, dpi_fit_core_forward, dpi_fit_core_backward) on a
host without a GPU: additions within ABI 8, every refusal returns its code and names its reason before any
device work.  CPU only."""
import ctypes

import pytest
import torch

import pis_fit_reference as R
from deeppicarditeration_amd import _lib, fit
from deeppicarditeration_amd.solution import PISGradNet

def _eq(nx=4):
    return R.make_equation((3, nx, [16], 1.0, 0.0, False, 1.0))


def _objective(nx=4):
    return fit.device_objective(0.0, torch.square, fit.FixedLossScaler(1.0), nx)


def test_pisgradnet_is_accepted_and_a_cpu_batch_is_no_torch_run():
    """g0 = OUProcessEquation.g: the network passes the checks; the CPU batch is then the error."""
    net = PISGradNet([16], 4, _eq().g)
    with pytest.raises(_lib.DPIError, match="no CPU fallback"):
        _objective()(net, torch.zeros(3, 5), torch.zeros(3, 5))
    with pytest.raises(_lib.DPIError, match="no CPU fallback"):  # the value kind too
        fit.device_objective(0.0, torch.square, None, 4)(net, torch.zeros(3, 5), torch.zeros(3, 5))


class _Other:
    def g(self, x):
        return x.sum(-1, keepdim=True)


def _channels_32():
    net = PISGradNet([16], 4, _eq().g)
    net.channels = 32
    return net


def _non_contiguous():
    net = PISGradNet([16], 4, _eq().g)
    net.nn_module[0].weight.data = torch.randn(68, 16).t()
    return net


@pytest.mark.parametrize("make, nx, named", [
    (lambda: PISGradNet([16], 4, lambda x: x.sum(-1, keepdim=True)), 4, "g0"),
    (lambda: PISGradNet([16], 4, _Other().g), 4, "OUProcessEquation"),
    (_channels_32, 4, "channels = 32"),
    (lambda: PISGradNet([8] * 5, 4, _eq().g), 4, "NETWORK.NEURONS"),
    (lambda: PISGradNet([16, 513], 4, _eq().g), 4, "NETWORK.NEURONS"),
    (lambda: PISGradNet([16], 129, _eq(129).g), 129, "nx = 129"),
    (lambda: PISGradNet([16], 4, _eq().g).double(), 4, "float64"),
    (_non_contiguous, 4, "non-contiguous"),
], ids=["lambda_g0", "other_equation", "channels", "depth", "width", "nx", "fp64", "non_contiguous"])
def test_refusals_name_pisgradnet_and_the_option(make, nx, named):
    """At the first batch, before the library is touched and before the device check (a CPU batch)."""
    with pytest.raises(NotImplementedError, match="PISGradNet") as ei:
        _objective(nx)(make(), torch.zeros(3, 1 + nx), torch.zeros(3, 1 + nx))
    assert named in str(ei.value)


def test_fp64_batch_is_refused_by_name():
    net = PISGradNet([16], 4, _eq().g)
    with pytest.raises(NotImplementedError, match="PISGradNet.*float64"):
        _objective()(net, torch.zeros(3, 5, dtype=torch.float64), torch.zeros(3, 5, dtype=torch.float64))


def test_the_other_scalers_stay_refused_whatever_the_network():
    with pytest.raises(NotImplementedError, match="SimpleLossScaler"):
        fit.device_objective(0.0, torch.square, fit.SimpleLossScaler(), 4)


# ---- the C entries

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


def _fwd(lib, nx=10, widths=(16, 16), tables=True, B=4, ws_bytes=None, tau_stride=64, x_stride=None, tau=PTR, q=PTR,
         hole=None):
    """dpi_fit_core_forward with non-null dummy device pointers (never dereferenced on a refusal)."""
    L = len(widths)
    if ws_bytes is None:
        ws_bytes = lib.dpi_fit_core_workspace_bytes(nx, L, _w(widths), B)
    tab = _tab(L + 1, hole) if tables else None
    return lib.dpi_fit_core_forward(nx, L, _w(widths), tab, tab, tau, tau_stride, PTR, nx if x_stride is None else x_stride,
                                    B, PTR, q, PTR, ws_bytes, None)


def _bwd(lib, nx=10, widths=(16, 16), tables=True, B=4, ws_bytes=None, e=PTR, r=PTR, dtau=PTR, hole=None):
    L = len(widths)
    if ws_bytes is None:
        ws_bytes = lib.dpi_fit_core_workspace_bytes(nx, L, _w(widths), B)
    good = _tab(L + 1)
    gtab = _tab(L + 1, hole) if tables else None
    return lib.dpi_fit_core_backward(nx, L, _w(widths), good, good, gtab, gtab, e, r, B, dtau, PTR, ws_bytes, None)


def test_symbols_are_additions_within_abi_8(lib):
    assert lib.dpi_abi_version() == 8 and _lib.DPI_ABI_VERSION == 8
    assert {"dpi_fit_core_workspace_bytes", "dpi_fit_core_forward", "dpi_fit_core_backward", "dpi_fit_gradients",
            "dpi_fit_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert lib.dpi_fit_core_workspace_bytes.restype is ctypes.c_size_t


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_caps_are_named_before_device_work(lib, call):
    assert call(lib, widths=(16, 513), ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED
    assert "513 > 512" in _lib.last_error()
    assert call(lib, widths=(8,) * 5, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED
    assert "5 hidden layers > 4" in _lib.last_error()
    assert call(lib, nx=129, ws_bytes=1 << 30) == _lib.DPI_ERR_UNSUPPORTED and "nx = 129 > 128" in _lib.last_error()
    assert call(lib, nx=0, ws_bytes=0) == _lib.DPI_ERR_ARG
    assert call(lib, B=-1, ws_bytes=0) == _lib.DPI_ERR_ARG
    assert call(lib, widths=(16, 0), ws_bytes=0) == _lib.DPI_ERR_ARG
    assert call(lib, tables=False) == _lib.DPI_ERR_ARG and "null pointer table" in _lib.last_error()
    assert call(lib, hole=1) == _lib.DPI_ERR_ARG and "layer 1" in _lib.last_error()
    need = lib.dpi_fit_core_workspace_bytes(10, 2, _w((16, 16)), 4)
    assert need > 0
    assert call(lib, ws_bytes=need - 1) == _lib.DPI_ERR_WORKSPACE and "workspace too small" in _lib.last_error()
    assert call(lib, widths=(512,) * 4, nx=128, ws_bytes=0) == _lib.DPI_ERR_WORKSPACE  # the caps themselves pass


def test_pointers_and_strides(lib):
    assert _fwd(lib, tau_stride=63) == _lib.DPI_ERR_ARG and "stride" in _lib.last_error()
    assert _fwd(lib, x_stride=9) == _lib.DPI_ERR_ARG and "stride" in _lib.last_error()
    assert _fwd(lib, tau=None) == _lib.DPI_ERR_ARG and "null tau" in _lib.last_error()
    assert _bwd(lib, e=None) == _lib.DPI_ERR_ARG and "null e" in _lib.last_error()
    assert _bwd(lib, dtau=None) == _lib.DPI_ERR_ARG


def test_empty_batch_launches_nothing(lib):
    w = _w((16, 16))
    assert lib.dpi_fit_core_forward(10, 2, w, None, None, None, 64, None, 10, 0, None, None, None, 0, None) == 0
    assert lib.dpi_fit_core_backward(10, 2, w, None, None, None, None, None, None, 0, None, None, 0, None) == 0


def test_workspace_steps_by_tiles_and_refused_shapes_have_none(lib):
    w = _w((512,) * 4)
    sizes = [lib.dpi_fit_core_workspace_bytes(100, 4, w, B) for B in (0, 1, 64, 65, 100, 128, 512)]
    assert sizes == sorted(sizes) and sizes[0] == 0
    assert sizes[1] == sizes[2] < sizes[3] == sizes[4] == sizes[5] < sizes[6]
    assert sizes[6] == 8 * sizes[1]
    assert lib.dpi_fit_core_workspace_bytes(100, 5, _w((8,) * 5), 64) == 0
    assert lib.dpi_fit_core_workspace_bytes(129, 1, _w((8,)), 64) == 0
    # the MLP fit's query is untouched by the core's caps
    assert lib.dpi_fit_workspace_bytes(101, 1, _w((512,)), 64) == 0
