"""Gradient-head networks (NETWORK.TYPE ValueGradient / OnlyGradient) at the boundaries that need no
GPU: the argument errors of dpi_net_create_mlp_head (they are checked before any device call), the
head classification of DeviceNet.from_module, and the runner's named refusals."""
import ctypes

import pytest
import torch

from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd import solution as S
from deeppicarditeration_amd.config import load_cfg
from deeppicarditeration_amd.runner import PicardRunner

NX = 7


def _create(widths, head, n_params, n_in=1 + NX):
    lib = L.load()
    w = (ctypes.c_int * len(widths))(*widths)
    buf = (ctypes.c_float * max(1, n_params))()
    return lib.dpi_net_create_mlp_head(n_in, len(widths), w, L.DPI_ACT_ELU, head, buf, n_params,
                                       ctypes.byref(ctypes.c_void_p()))


def _count(widths, n_out, n_in=1 + NX):
    dims = [n_in] + list(widths)
    return sum(dims[i + 1] * (dims[i] + 1) for i in range(len(widths))) + n_out * (dims[-1] + 1)


@pytest.mark.parametrize("head,n_out,word", [(L.DPI_HEAD_VALUE_GRADIENT, NX, "1 + nx"), (L.DPI_HEAD_VALUE_GRADIENT, 1, "1 + nx"),
                                             (L.DPI_HEAD_GRADIENT, 1 + NX, "nx output rows"), (L.DPI_HEAD_GRADIENT, 1, "nx output rows")])
def test_parameter_count_must_match_the_head(head, n_out, word):
    assert _create([16, 16], head, _count([16, 16], n_out)) == L.DPI_ERR_ARG
    assert "parameter count" in L.last_error() and word in L.last_error()


def test_value_head_is_create_mlp():
    assert _create([16, 16], L.DPI_HEAD_VALUE, _count([16, 16], NX)) == L.DPI_ERR_ARG
    assert "parameter count" in L.last_error()


@pytest.mark.parametrize("head", [-1, 3, 17])
def test_unknown_head_code(head):
    assert _create([16, 16], head, _count([16, 16], 1 + NX)) == L.DPI_ERR_ARG
    assert "DPI_HEAD_VALUE_GRADIENT" in L.last_error()


@pytest.mark.parametrize("widths,word", [([16] * 9, "8"), ([16, 257], "256")])
@pytest.mark.parametrize("head", [L.DPI_HEAD_VALUE_GRADIENT, L.DPI_HEAD_GRADIENT])
def test_upload_caps(widths, word, head):
    assert _create(widths, head, 1) == L.DPI_ERR_UNSUPPORTED and word in L.last_error()


def test_header_and_binding_name_the_heads():
    assert (L.DPI_HEAD_VALUE, L.DPI_HEAD_VALUE_GRADIENT, L.DPI_HEAD_GRADIENT) == (0, 1, 2)
    assert "dpi_net_create_mlp_head" in L.SIGNATURES and L.DPI_ABI_VERSION == 8


def test_head_classification():
    assert S.head_of(1, NX) == L.DPI_HEAD_VALUE
    assert S.head_of(1 + NX, NX) == L.DPI_HEAD_VALUE_GRADIENT
    assert S.head_of(NX, NX) == L.DPI_HEAD_GRADIENT
    assert S.head_of(1, 1) == L.DPI_HEAD_VALUE  # nx = 1: one output is a Value net
    for n_out in (0, 2, NX - 1, NX + 2):
        with pytest.raises(ValueError, match=r"1 \(Value\).*ValueGradient.*OnlyGradient"):
            S.head_of(n_out, NX)
    out = torch.arange(2.0 * (1 + NX)).reshape(2, 1 + NX)
    u, ux = S.head_columns(out, NX)
    assert torch.equal(u, out[:, :1]) and torch.equal(ux, out[:, 1:])
    u, ux = S.head_columns(out[:, 1:], NX)
    assert torch.equal(u, torch.zeros(2, 1)) and torch.equal(ux, out[:, 1:])
    assert S.head_columns(out[:, :1], NX)[1] is None


def test_from_module_refuses_an_illegal_output_width():
    m = S.construct_mlp(1 + NX, 3, [8], ["Tanh"], None)
    with pytest.raises(ValueError, match="output width 3"):
        S.DeviceNet.from_module(m, 1 + NX)


YAML = """NAME: {name}
EQUATION:
  cls: Cha
  kwargs: {{nx: 6, alpha: 1.0, k: 5.0, T: 1.0}}
PICARD: {{N: 1}}
FORCE: true
TRAIN: {{SUPERVISE_HESSIAN: {hess}}}
NETWORK:
  TYPE: {typ}
  PISGRADNET: {pis}
  NEURONS: [8, 8]
  ACTIVATIONS: [Tanh, Tanh]
"""


def _runner(tmp_path, typ, pis=False, hess=False):
    f = tmp_path / "c.yaml"
    f.write_text(YAML.format(name=tmp_path / "run", typ=typ, pis=str(pis).lower(), hess=str(hess).lower()))
    return PicardRunner(load_cfg(str(f)), device="cpu")


@pytest.mark.parametrize("typ,out", [("Value", 1), ("ValueGradient", 7), ("OnlyGradient", 6)])
def test_runner_builds_the_head(tmp_path, typ, out):
    r = _runner(tmp_path, typ)
    assert r.output_dim == out and r.u_current.output_dim == out
    net = r.new_network()
    assert [l for l in net if isinstance(l, torch.nn.Linear)][-1].out_features == out


def test_runner_refusals(tmp_path):
    with pytest.raises(ValueError, match="Unknown network type"):
        _runner(tmp_path, "Gradient")
    with pytest.raises(NotImplementedError, match="PISGRADNET"):
        _runner(tmp_path, "OnlyGradient", pis=True)
    with pytest.raises(NotImplementedError, match="SUPERVISE_HESSIAN"):
        _runner(tmp_path, "ValueGradient", hess=True)
