"""The PISGradNet core's kernels (k_fit_core_fwd, k_fit_core_bwd, k_fit_core_wgrad of csrc/dpi_fit.h, DESIGN.md
§5.1) through their C entries, every output on its own against the fp64 restatement of the same fp32 inputs:
sp, q = d sp / d x, dtau and each dW_l, db_l of nn_module, on the core's case table (tests/pis_fit_reference.py,
CORE_CASES x MODES), judged against what two honest fp32 evaluations of the same primitive are off by; row
strides past the row length; and the call forms a missing cotangent takes.

Measured on an MI355X over the 315 outputs of the 36 case x mode pairs (DESIGN.md §5.1 has the ranges per
output kind): e_hip 0 - 5.7e-7 against E_case 1.3e-7 - 1.2e-6, e_hip / max(E_case, 2^-24) at most 1.38 (dtau at
B = 1, nx = 128, [1], q_cot_only)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pis_fit_reference as R
from deeppicarditeration_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 2e-6  # of E_case; tests/test_pis_core_reference.py holds the CPU's fp32 evaluations to the same one
PAIRS = [(k, m) for k in range(len(R.CORE_CASES)) for m in R.MODES]
PAIR_IDS = [f"{R.CORE_IDS[k]}-{m}" for k, m in PAIRS]


@functools.lru_cache(maxsize=None)
def _fp64(k, mode):
    """The yardstick, computed once per case and mode and never written to."""
    return R.core_outputs(R.core_case(k, mode), mode)


def _padded(a, pad):
    """a (B, n) on the device as a view of a (B, n + pad) buffer whose padding holds NaN."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(a)
    return buf[:, :a.shape[1]]


def _call(k, inputs, mode, tau_pad=0, x_pad=0):
    """dpi_fit_core_forward + dpi_fit_core_backward on the inputs of R.core_case.  Returns [sp, q or None,
    dtau, dW_1 .., db_1 ..] as fp32 CPU tensors; every output was pre-filled with NaN."""
    B, nx, widths = R.CORE_CASES[k]
    Ws, bs, tau, x, e, r = inputs
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(a).to(DEV).contiguous()  # noqa: E731
    Wd, bd = [dev(W) for W in Ws], [dev(b) for b in bs]
    tau_d, x_d, e_d = _padded(tau, tau_pad), _padded(x, x_pad), dev(e)
    r_d = None if r is None else dev(r)
    assert tau_d.stride(0) == 64 + tau_pad and x_d.stride(0) == nx + x_pad
    cw = (ctypes.c_int * len(widths))(*widths)
    need = int(lib.dpi_fit_core_workspace_bytes(nx, len(widths), cw, B))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    sp, q, dtau = nan(B, 1), nan(B, nx) if mode != "value" else None, nan(B, 64)
    gW, gb = [nan(*W.shape) for W in Ws], [nan(*b.shape) for b in bs]
    tab = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.dpi_fit_core_forward(nx, len(widths), cw, tab(Wd), tab(bd), tau_d.data_ptr(), tau_d.stride(0),
                                        x_d.data_ptr(), x_d.stride(0), B, sp.data_ptr(),
                                        None if q is None else q.data_ptr(), ws.data_ptr(), need, st), "forward")
    _lib.check(lib.dpi_fit_core_backward(nx, len(widths), cw, tab(Wd), tab(bd), tab(gW), tab(gb), e_d.data_ptr(),
                                         None if r_d is None else r_d.data_ptr(), B, dtau.data_ptr(), ws.data_ptr(),
                                         need, st), "backward")
    torch.cuda.synchronize()
    return [None if o is None else o.cpu() for o in [sp, q, dtau] + gW + gb]


def _same_bits(a, b):
    return all((u is None and v is None) or torch.equal(u.view(torch.int32), v.view(torch.int32))
               for u, v in zip(a, b))


@pytest.mark.parametrize("k,mode", PAIRS, ids=PAIR_IDS)
def test_outputs_against_fp64(k, mode):
    """Every output's rel-L2 e_hip <= 4 max(E_case, 2^-24), E_case the largest error of any output of the
    case over two fp32 evaluations of the reference: torch fp32 autograd of the same primitive on this GPU and
    the numpy restatement in fp32 on the CPU; E_case <= 2e-6, so the bar is never above 8e-6.  The pool is
    the case's, not the tensor's: two honest fp32 evaluations differ by up to 10.6 x on a three-element bias
    gradient, never by 4 x of the case's worst output.  An output whose fp64 value is exactly zero comes
    back exactly zero; all come back finite over their NaN fill."""
    inputs, want, names = R.core_case(k, mode), _fp64(k, mode), R.core_names(k)
    pool = (R.core_errors(R.torch_core(inputs, mode, torch.float32, DEV), want)
            + R.core_errors(R.core_outputs(inputs, mode, np.float32), want))
    e_case = max(e for e in pool if e is not None)
    got = _call(k, inputs, mode)
    assert len(got) == len(want) == len(names)
    errs = {}
    for name, g, w in zip(names, got, want):
        assert (g is None) == (w is None), name
        if g is None:
            continue
        g = g.numpy()
        assert g.shape == w.shape and np.isfinite(g).all(), name
        if not np.any(w):
            assert not np.any(g), name
            continue
        errs[name] = R.rel_l2(g, w)
        print(f"FIT_CORE {R.CORE_IDS[k]} {mode} {name} e_hip {errs[name]:.3e} E_case {e_case:.3e}")
    assert e_case <= CAP, e_case
    bar = 4 * max(e_case, 2.0 ** -24)
    assert all(e <= bar for e in errs.values()), (bar, {n: e for n, e in errs.items() if e > bar})


STRIDED = [R.CORE_CASES.index(c) for c in [(65, 10, [64] * 4), (129, 127, [17, 511])]]


@pytest.mark.parametrize("k", STRIDED, ids=[R.CORE_IDS[k] for k in STRIDED])
def test_row_strides(k):
    """tau a view of a (B, 80) buffer and x of a (B, nx + 5) buffer, the padding NaN: bit-identical to the
    contiguous call."""
    inputs = R.core_case(k, "grad")
    flat, strided = _call(k, inputs, "grad"), _call(k, inputs, "grad", tau_pad=16, x_pad=5)
    assert all(bool(torch.isfinite(o).all()) for o in strided)
    assert _same_bits(flat, strided)


def test_cotangent_forms():
    """A backward without r after a forward that formed q skips pass 3 as the value mode does: dW, db and dtau
    are bit-identical to value mode's.  e = 0 is no special case: q_cot_only equals grad with the same r and a
    separately allocated e of zeros, to the bit."""
    k = R.CORE_CASES.index((100, 3, [130, 70]))
    value, sp_only = _call(k, R.core_case(k, "value"), "value"), _call(k, R.core_case(k, "sp_cot_only"), "sp_cot_only")
    assert value[1] is None and sp_only[1] is not None and bool(torch.isfinite(sp_only[1]).all())
    assert _same_bits([value[0]] + value[2:], [sp_only[0]] + sp_only[2:])
    Ws, bs, tau, x, e, r = R.core_case(k, "grad")
    assert np.any(e)
    zeros = np.zeros((R.CORE_CASES[k][0], 1), np.float32)
    q_only = R.core_case(k, "q_cot_only")
    assert not np.any(q_only[4]) and np.array_equal(q_only[5], r)
    assert _same_bits(_call(k, q_only, "q_cot_only"), _call(k, (Ws, bs, tau, x, zeros, r), "grad"))
