"""The layer-wise form of the PISGradNet core (TRAIN.CORE_FORM: layers; k_fit_layer of csrc/dpi_fit_layers.h,
DESIGN.md §5.1) on the GPU, through dpi_fit_core_layers_forward / _backward: every output on its own against
the fp64 restatement by the measure and the bar of tests/test_gpu_pis_core.py, on its case table plus three
shapes on the edges of the 16 x 16 x 4 MFMA tile; a workspace pre-filled with NaN; row strides; reproducibility
and canaries; the cotangent forms; then through fit.device_objective by the protocol of
tests/test_gpu_pis_fit.py, and `picard train` end to end.

Measured on an MI355X over the 428 outputs of the 48 case x mode pairs ("The layer-wise form", has
the ranges per output kind): e_hip 0 - 1.1e-6 against E_case 1.3e-7 - 1.2e-6, e_hip / max(E_case, 2^-24) at most
2.04 (dW1 at B = 1, nx = 128, [1], value), 0.99 on the three extra shapes.  Through the objective: e_hip 2.8e-6 -
2.9e-5, e_hip / e_32 0.66 - 1.11, on nn_module's tensors alone 0.60 - 1.11; iteration 1's first-step losses of
the two backends were equal to the last bit."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import pis_fit_reference as R
from deeppicarditeration_amd import _lib, fit, runner as runner_module
from deeppicarditeration_amd.config import load_cfg
from deeppicarditeration_amd.runner import PicardRunner

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 2e-6  # of E_case, as tests/test_gpu_pis_core.py
CANARY = 4 << 20

# (B, nx, hidden widths) on the MFMA tile edges: one row past a 16-row fragment, n0 = 66, widths one under 16 and
# one past 32; one row under the 64-row tile, n0 = 69, exact and inexact widths; no edge anywhere
EXTRA = [(17, 2, [15, 33]), (63, 5, [48, 16, 31]), (16, 4, [16, 16])]
SHAPES = list(R.CORE_CASES) + EXTRA
SHAPE_IDS = list(R.CORE_IDS) + [f"{len(R.CORE_CASES) + j}-B{c[0]}-nx{c[1]}-{'x'.join(map(str, c[2]))}"
                                for j, c in enumerate(EXTRA)]
PAIRS = [(k, m) for k in range(len(SHAPES)) for m in R.MODES]
PAIR_IDS = [f"{SHAPE_IDS[k]}-{m}" for k, m in PAIRS]


def _inputs(k, mode):
    """R.core_case(k, mode) on the case table; for the extra shapes k = 9, 10, 11 the same recipe restated:
    default_rng(100 + k), W = (U(-1, 1) + N(0, 1)) / sqrt(fan_in), b = U(-1, 1) / sqrt(fan_in) + 0.3 N(0, 1), tau,
    x, e, r standard normals, drawn in that order."""
    if k < len(R.CORE_CASES):
        return R.core_case(k, mode)
    B, nx, widths = SHAPES[k]
    rng = np.random.default_rng(100 + k)
    n = [R.NT + nx] + list(widths) + [nx]
    fan = list(zip(n[1:], n[:-1]))
    Ws = [((rng.uniform(-1, 1, (o, i)) + rng.standard_normal((o, i))) * i ** -0.5).astype(np.float32) for o, i in fan]
    bs = [(rng.uniform(-1, 1, o) * i ** -0.5 + 0.3 * rng.standard_normal(o)).astype(np.float32) for o, i in fan]
    tau, x, e, r = (rng.standard_normal((B, m)).astype(np.float32) for m in (R.NT, nx, 1, nx))
    if mode == "q_cot_only":
        e = np.zeros_like(e)
    if mode in ("value", "sp_cot_only"):
        r = None
    return Ws, bs, tau, x, e, r


def _names(k):
    L1 = len(SHAPES[k][2]) + 1
    return ["sp", "q", "dtau"] + [f"dW{l}" for l in range(1, L1 + 1)] + [f"db{l}" for l in range(1, L1 + 1)]


@functools.lru_cache(maxsize=None)
def _fp64(k, mode):
    """The yardstick, computed once per case and mode and never written to."""
    return R.core_outputs(_inputs(k, mode), mode)


def _padded(a, pad):
    """a (B, n) on the device as a view of a (B, n + pad) buffer whose padding holds NaN."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(a)
    return buf[:, :a.shape[1]]


def _guarded(shape, fill):
    """A float tensor of `shape` filled with `fill` and the 4 MB canary behind it, from one allocation."""
    n = 4 * int(np.prod(shape))
    buf = torch.full((n + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    t = buf[:n].view(torch.float32).view(*shape)
    t.fill_(fill)
    return t, buf[n:]


def _call(k, inputs, mode, tau_pad=0, x_pad=0, ws_fill=float("nan")):
    """dpi_fit_core_layers_forward + _backward on `inputs`.  Returns [sp, q or None, dtau, dW_1 .., db_1 ..] as
    fp32 CPU tensors; every output was pre-filled with NaN and the workspace with ws_fill, and the canaries
    behind all of them are checked."""
    B, nx, widths = SHAPES[k]
    Ws, bs, tau, x, e, r = inputs
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(a).to(DEV).contiguous()  # noqa: E731
    Wd, bd = [dev(W) for W in Ws], [dev(b) for b in bs]
    tau_d, x_d, e_d = _padded(tau, tau_pad), _padded(x, x_pad), dev(e)
    r_d = None if r is None else dev(r)
    assert tau_d.stride(0) == 64 + tau_pad and x_d.stride(0) == nx + x_pad
    cw = (ctypes.c_int * len(widths))(*widths)
    need = int(lib.dpi_fit_core_layers_workspace_bytes(nx, len(widths), cw, B))
    assert need > 0 and need % 4 == 0
    guards = []

    def buf(shape, fill=float("nan")):
        t, g = _guarded(shape, fill)
        guards.append(g)
        return t

    ws = buf((need // 4,), ws_fill)
    sp, q, dtau = buf((B, 1)), buf((B, nx)) if mode != "value" else None, buf((B, 64))
    gW, gb = [buf(W.shape) for W in Ws], [buf(b.shape) for b in bs]
    tab = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.dpi_fit_core_layers_forward(nx, len(widths), cw, tab(Wd), tab(bd), tau_d.data_ptr(),
                                               tau_d.stride(0), x_d.data_ptr(), x_d.stride(0), B, sp.data_ptr(),
                                               None if q is None else q.data_ptr(), ws.data_ptr(), need, st),
               "forward")
    _lib.check(lib.dpi_fit_core_layers_backward(nx, len(widths), cw, tab(Wd), tab(bd), tab(gW), tab(gb),
                                                e_d.data_ptr(), None if r_d is None else r_d.data_ptr(), B,
                                                dtau.data_ptr(), ws.data_ptr(), need, st), "backward")
    torch.cuda.synchronize()
    assert all(bool((g == 0xA5).all()) for g in guards), "a canary behind the workspace or an output was written"
    return [None if o is None else o.cpu() for o in [sp, q, dtau] + gW + gb]


def _same_bits(a, b):
    return all((u is None and v is None) or torch.equal(u.view(torch.int32), v.view(torch.int32))
               for u, v in zip(a, b))


def _finite(outs):
    return all(o is None or bool(torch.isfinite(o).all()) for o in outs)


@pytest.mark.parametrize("k,mode", PAIRS, ids=PAIR_IDS)
def test_outputs_against_fp64(k, mode):
    """Every output's rel-L2 e_hip <= 4 max(E_case, 2^-24), E_case the largest error of any output of the case
    over torch fp32 autograd of the same primitive on this GPU and the numpy restatement in fp32; E_case <= 2e-6
    is a condition on the draws.  An output whose fp64 value is exactly zero comes back exactly zero; all come
    back finite over their NaN fill."""
    inputs, want, names = _inputs(k, mode), _fp64(k, mode), _names(k)
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
        print(f"FIT_LAYERS {SHAPE_IDS[k]} {mode} {name} e_hip {errs[name]:.3e} E_case {e_case:.3e}")
    assert e_case <= CAP, e_case
    bar = 4 * max(e_case, 2.0 ** -24)
    assert all(e <= bar for e in errs.values()), (bar, {n: e for n, e in errs.items() if e > bar})


NAN_WS = [SHAPES.index(c) for c in [(65, 1, [3]), (129, 127, [17, 511]), (17, 2, [15, 33])]]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("k", NAN_WS, ids=[SHAPE_IDS[k] for k in NAN_WS])
def test_nan_filled_workspace(k, mode):
    """No launch reads a workspace element that no earlier launch of the same forward / backward pair wrote: over
    a workspace of NaN every output is finite and bit-identical to the run over a workspace of zeros."""
    inputs = _inputs(k, mode)
    nan, zero = _call(k, inputs, mode), _call(k, inputs, mode, ws_fill=0.0)
    assert _finite(nan) and _finite(zero)
    assert _same_bits(nan, zero)


STRIDED = [SHAPES.index(c) for c in [(65, 10, [64] * 4), (129, 127, [17, 511])]]


@pytest.mark.parametrize("k", STRIDED, ids=[SHAPE_IDS[k] for k in STRIDED])
def test_row_strides(k):
    """tau a view of a (B, 80) buffer and x of a (B, nx + 5) buffer, the padding NaN: bit-identical to the
    contiguous call."""
    inputs = _inputs(k, "grad")
    flat, strided = _call(k, inputs, "grad"), _call(k, inputs, "grad", tau_pad=16, x_pad=5)
    assert _finite(strided)
    assert _same_bits(flat, strided)


PARTIAL = [SHAPES.index(c) for c in [(1, 3, [16]), (65, 10, [64] * 4), (100, 3, [130, 70])]]


@pytest.mark.parametrize("k", PARTIAL, ids=[SHAPE_IDS[k] for k in PARTIAL])
def test_reproducible_and_in_bounds(k):
    """B = 1, 65 and 100: two forward + backward calls are bit-identical in every output; the 4 MB canaries behind
    the workspace and behind every output stay intact (checked by _call)."""
    inputs = _inputs(k, "grad")
    first, second = _call(k, inputs, "grad"), _call(k, inputs, "grad")
    assert _finite(first)
    assert _same_bits(first, second)


def test_cotangent_forms():
    """A backward without r after a forward that formed q skips pass 3 as the value mode does: dW, db and dtau
    are bit-identical to value mode's.  e = 0 is no special case: q_cot_only equals grad with the same r and a
    separately allocated e of zeros, to the bit."""
    k = SHAPES.index((100, 3, [130, 70]))
    value, sp_only = _call(k, _inputs(k, "value"), "value"), _call(k, _inputs(k, "sp_cot_only"), "sp_cot_only")
    assert value[1] is None and sp_only[1] is not None and bool(torch.isfinite(sp_only[1]).all())
    assert _same_bits([value[0]] + value[2:], [sp_only[0]] + sp_only[2:])
    Ws, bs, tau, x, e, r = _inputs(k, "grad")
    assert np.any(e)
    zeros = np.zeros((SHAPES[k][0], 1), np.float32)
    q_only = _inputs(k, "q_cot_only")
    assert not np.any(q_only[4]) and np.array_equal(q_only[5], r)
    assert _same_bits(_call(k, q_only, "q_cot_only"), _call(k, (Ws, bs, tau, x, zeros, r), "grad"))


# ---- through the objective (the protocol of tests/test_gpu_pis_fit.py)

def _device_objective(case, clip):
    beta, c, nx = case[4], case[6], case[1]
    return fit.device_objective(beta, R.loss_fn_of(clip), None if c <= 1e-9 else fit.FixedLossScaler(c), nx,
                                core_form="layers")


def _errors(got, want):
    """The largest per-tensor rel-L2 of the gradients, and the loss's relative error."""
    return R.worst_rel_l2(got[1], want[1]), abs(got[0] - want[0]) / abs(want[0])


@pytest.mark.parametrize("k", range(len(R.CASES)), ids=R.IDS)
def test_objective_parity_with_fp64_autograd(k):
    """e_hip <= 4 e_32 and e_hip < 1e-4 against torch fp64 autograd on the CPU, e the largest of the per-tensor
    rel-L2 of all PISGradNet parameter gradients and the loss's relative error, e_32 today's torch fp32 objective
    on this GPU; and the same factor over the nn_module.* tensors alone."""
    case = R.CASES[k]
    clip = R.make_batch(k)[2]
    want = R.torch_fp64(k)
    t32 = R.torch_result(k, torch.float32, DEV)
    net = R.make_net(case, torch.float32, DEV)
    hip = R.run(_device_objective(case, clip), net, k, torch.float32, DEV)
    (g_hip, l_hip), (g_32, l_32) = _errors(hip, want), _errors(t32, want)
    e_hip, e_32 = max(g_hip, l_hip), max(g_32, l_32)
    names = R.param_names(case)
    t_hip, t_32 = R.tensor_errors(hip[1], want[1]), R.tensor_errors(t32[1], want[1])
    core = [n.startswith("nn_module.") for n in names]  # the tensors the HIP core computes
    assert any(core) and not all(core)
    nn_hip, nn_32 = (max(e for e, c in zip(t, core) if c) for t in (t_hip, t_32))
    print(f"PIS_LAYERS_PARITY {R.IDS[k]} e_hip {e_hip:.3e} e_32 {e_32:.3e} (grad {g_hip:.3e} / {g_32:.3e}, loss "
          f"{l_hip:.3e} / {l_32:.3e}; nn_module {nn_hip:.3e} / {nn_32:.3e})")
    assert e_hip <= 4 * e_32 and e_hip < 1e-4, (e_hip, e_32)
    assert nn_hip <= 4 * nn_32, (nn_hip, nn_32)


def test_picard_train_hjb_with_the_layer_wise_core(tmp_path, monkeypatch):
    """`picard train` on the HJB keys of tests/test_gpu_pis_fit.py (nx = 10, NEURONS [64] * 4, two Picard
    iterations) with TRAIN.BACKEND hip TRAIN.CORE_FORM layers and under the torch backend from the same
    torch.manual_seed: finite checkpoints, and iteration 1's first-step losses agree to 1e-4 relative."""
    from test_gpu_pis_fit import HJB, _MEAN
    first = {}
    steps = runner_module.train_steps

    def recording(net, objective, opt, batches, sched=None):
        losses = steps(net, objective, opt, batches, sched)
        first.setdefault(backend, float(losses[0]))
        return losses

    monkeypatch.setattr(runner_module, "train_steps", recording)
    forms = []

    class Plan(fit._PISPlan):
        def __init__(self, net, nx, core_form="tiles"):
            forms.append(core_form)
            super().__init__(net, nx, core_form)

    monkeypatch.setattr(fit, "_PISPlan", Plan)
    for backend in ("hip", "torch"):
        f = tmp_path / f"hjb_{backend}.yaml"
        f.write_text(HJB.format(name=tmp_path / f"run_{backend}", backend=backend, mean=_MEAN, var=[[2.0] * 10] * 2))
        torch.manual_seed(123)
        cfg = load_cfg(str(f), ["TRAIN.CORE_FORM", "layers"] if backend == "hip" else None)
        assert cfg.TRAIN.CORE_FORM == ("layers" if backend == "hip" else "tiles")
        runner = PicardRunner(cfg)
        runner.run()
        assert [h["iter"] for h in runner.history] == [1, 2]
        lines = [json.loads(l) for l in (tmp_path / f"run_{backend}" / "history.jsonl").read_text().splitlines()]
        assert [l["fit"] for l in lines] == ["gradient"] * 2 and [l["fit_backend"] for l in lines] == [backend] * 2
        for i in (1, 2):
            sd = torch.load(tmp_path / f"run_{backend}" / f"model_{i}.pt", weights_only=True)
            assert all(torch.isfinite(v).all() for v in sd.values())
    assert forms and set(forms) == {"layers"}, forms  # the hip runs took the layer-wise entries; torch built no plan
    print("PIS_LAYERS_TRAIN first-step loss of iteration 1", first)
    assert abs(first["hip"] - first["torch"]) <= 1e-4 * abs(first["torch"]), first
