"""The shell of the device fit of a PISGradNet (TRAIN.PIS_SHELL: hip; csrc/dpi_fit_shell.h) on the
GPU: every output of the three C stages on its own against the fp64 restatement of the same fp32 inputs
(tests/pis_shell_reference.py), judged against what two honest fp32 evaluations are off by; row strides;
reproducibility, canaries and overwrite semantics; parity of the whole objective with torch fp64 autograd under
both forms of the core; a 20-step Adam trajectory; and `picard train` end to end.

Measured on an MI355X (profiles/pis_shell/test_gpu_pis_shell.txt): over the stage table e_hip is at
most 3.1e-6 and e_hip / max(E_case, 2^-24) at most 0.39 (res_x at nx = 128, 8 components), E_case 1.4e-6 - 3.1e-6;
through the objective e_hip 4.1e-7 - 2.1e-5 against e_32 2.8e-6 - 2.9e-5, e_hip / e_32 at most 1.49; the
trajectory distances are 1.03e-3 (hip) and 2.02e-3 (torch fp32) at |w| = 32."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import pis_fit_reference as R
import pis_shell_reference as S
from deeppicarditeration_amd import _lib, fit, runner as runner_module
from deeppicarditeration_amd.config import load_cfg
from deeppicarditeration_amd.runner import PicardRunner

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 5e-6  # of E_case; tests/test_pis_shell_reference.py holds the CPU's fp32 evaluations to the same one
PAIRS = [(k, m) for k in range(len(S.CASES)) for m in S.MODES]
PAIR_IDS = [f"{S.IDS[k]}-{m}" for k, m in PAIRS]
CANARY = 4 << 20


@functools.lru_cache(maxsize=None)
def _fp64(k, mode):
    """The yardstick, computed once per case and mode and never written to."""
    return S.stage_outputs(k, mode)


def _padded(a, pad):
    """a (B, n) on the device as a view of a (B, n + pad) buffer whose padding holds NaN."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(a)
    return buf[:, :a.shape[1]]


def _guarded(shape):
    """(view of `shape` pre-filled with NaN, the whole buffer) with a 4 MB canary behind the view."""
    n = 4 * int(np.prod(shape))
    buf = torch.full((n + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    view = buf[:n].view(torch.float32).view(*shape)
    view.fill_(float("nan"))
    return view, buf


def _call(k, mode, tx_pad=0, y_pad=0):
    """The three C stages on the inputs of S.stage_case(k): the forward; the loss on the forward's s, res, res_x
    and the drawn sp, q; the backward on the drawn taubar, sbar.  Every output NaN-prefilled with a canary behind
    it, the workspace NaN-filled.  Returns the outputs in S.stage_names order (fp32 CPU tensors; None where the
    mode forms none) and the guard buffers with their payload sizes."""
    B, nx, depth, T, ncomp, beta, _ = S.CASES[k]
    c = S.stage_case(k)
    grad = mode == "grad"
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(a).to(DEV).contiguous()  # noqa: E731
    P = [dev(p) for p in c["P"]]
    coeff = dev(c["coeff"])
    tx, y = _padded(c["tx"], tx_pad), _padded(c["y"], y_pad)
    sp, q, taubar, sbar_in = dev(c["sp"]), dev(c["q"]), dev(c["taubar"]), dev(c["sbar"])
    problem = c["net"].g0.__self__.dpi_problem()
    need = int(lib.dpi_fit_shell_workspace_bytes(nx, depth, B))
    assert need > 0
    guards = []

    def out(*shape):
        view, buf = _guarded(shape)
        guards.append((buf, 4 * view.numel()))
        return view

    ws = out(need // 4)
    tau, s, res, losses, e, sbar = out(B, 64), out(B, 1), out(B, 1), out(2 + nx), out(B, 1), out(B, 1)
    res_x, r = (out(B, nx), out(B, nx)) if grad else (None, None)
    grads = [out(*p.shape) for p in P]
    tab = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.dpi_fit_shell_forward(problem, T, nx, depth, coeff.data_ptr(), tab(P), tx.data_ptr(), tx.stride(0),
                                         B, int(grad), tau.data_ptr(), s.data_ptr(), res.data_ptr(), ptr(res_x),
                                         ws.data_ptr(), need, st), "forward")
    _lib.check(lib.dpi_fit_shell_loss(nx, sp.data_ptr(), q.data_ptr() if grad else None, s.data_ptr(), res.data_ptr(),
                                      ptr(res_x), tx.data_ptr(), tx.stride(0), y.data_ptr(), y.stride(0), B, beta,
                                      _lib.DPI_FIT_LOSS_SQUARE if c["clip"] is None else _lib.DPI_FIT_LOSS_CLIP,
                                      c["clip"] or 0.0, S.KAPPA if grad else 0.0, losses.data_ptr(), e.data_ptr(),
                                      ptr(r), sbar.data_ptr(), ws.data_ptr(), need, st), "loss")
    _lib.check(lib.dpi_fit_shell_backward(nx, depth, tab(P), tab(grads), taubar.data_ptr(), sbar_in.data_ptr(), B,
                                          ws.data_ptr(), need, st), "backward")
    torch.cuda.synchronize()
    outs = [None if o is None else o.cpu() for o in [tau, s, res, res_x, losses, e, r, sbar] + grads]
    return outs, guards


def _same_bits(a, b):
    return all((u is None and v is None) or torch.equal(u.view(torch.int32), v.view(torch.int32))
               for u, v in zip(a, b))


@pytest.mark.parametrize("k,mode", PAIRS, ids=PAIR_IDS)
def test_stage_outputs_against_fp64(k, mode):
    """Every output's rel-L2 e_hip <= 4 max(E_case, 2^-24), E_case the largest error of any output of the case
    over two fp32 evaluations of the reference: torch fp32 on this GPU and the numpy restatement in fp32 on the
    CPU; E_case <= 5e-6, so the bar is never above 2e-5.  An output whose fp64 value is exactly zero comes back
    exactly zero; all come back finite over their NaN fill."""
    want, names = _fp64(k, mode), S.stage_names(k)
    pool = (S.stage_errors(S.torch_stages(k, mode, torch.float32, DEV), want)
            + S.stage_errors(S.stage_outputs(k, mode, np.float32), want))
    e_case = max(e for e in pool if e is not None)
    got, _ = _call(k, mode)
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
        print(f"PIS_SHELL {S.IDS[k]} {mode} {name} e_hip {errs[name]:.3e} E_case {e_case:.3e}")
    assert e_case <= CAP, e_case
    bar = 4 * max(e_case, 2.0 ** -24)
    assert all(e <= bar for e in errs.values()), (bar, {n: e for n, e in errs.items() if e > bar})


STRIDED = [2, 3]


@pytest.mark.parametrize("k", STRIDED, ids=[S.IDS[k] for k in STRIDED])
def test_row_strides(k):
    """tx a view of a (B, 1 + nx + 7) buffer and y of a (B, 1 + nx + 5) buffer, the padding NaN: bit-identical to
    the contiguous call."""
    flat, strided = _call(k, "grad")[0], _call(k, "grad", tx_pad=7, y_pad=5)[0]
    assert all(bool(torch.isfinite(o).all()) for o in strided)
    assert _same_bits(flat, strided)


PARTIAL = [0, 2, 4]


@pytest.mark.parametrize("k", PARTIAL, ids=[S.IDS[k] for k in PARTIAL])
def test_c_calls_are_deterministic_overwrite_and_stay_in_bounds(k):
    """Partial-tile shapes (B = 1, 65, 100), both modes: two runs are bit-identical; the 4 MB canaries behind the
    workspace and every output are intact; NaN-prefilled outputs over a NaN-filled workspace come back finite;
    smooth_net's last bias gradient and the rows >= 1 of its last weight gradient are exactly 0.0."""
    names = S.stage_names(k)
    for mode in S.MODES:
        (a, guards), (b, _) = _call(k, mode), _call(k, mode)
        for buf, n in guards:
            assert bool((buf[n:] == 0xA5).all())
        assert all(o is None or bool(torch.isfinite(o).all()) for o in a)
        assert _same_bits(a, b)
        depth = S.CASES[k][2]
        last_w = a[names.index(f"d smooth_net.{2 * (depth + 1)}.weight")]
        last_b = a[names.index(f"d smooth_net.{2 * (depth + 1)}.bias")]
        assert bool((last_b == 0).all()) and bool((last_w[1:] == 0).all()) and bool((last_w[0] != 0).any())


def _device_objective(case, clip, core_form):
    beta, c, nx = case[4], case[6], case[1]
    return fit.device_objective(beta, R.loss_fn_of(clip), None if c <= 1e-9 else fit.FixedLossScaler(c), nx,
                                core_form=core_form, pis_shell="hip")


@pytest.mark.parametrize("form", ("tiles", "layers"))
@pytest.mark.parametrize("k", range(len(R.CASES)), ids=R.IDS)
def test_parity_with_fp64_autograd(k, form):
    """e_hip <= 4 e_32 and e_hip < 1e-4, e the largest of the per-tensor rel-L2 of all PISGradNet parameter
    gradients and the loss's relative error (the measure of tests/test_gpu_pis_fit.py); the same factor over the
    time networks' tensors alone, which are now HIP's, and over nn_module.* alone."""
    case = R.CASES[k]
    clip = R.make_batch(k)[2]
    want = R.torch_fp64(k)
    t32 = R.torch_result(k, torch.float32, DEV)
    net = R.make_net(case, torch.float32, DEV)
    hip = R.run(_device_objective(case, clip, form), net, k, torch.float32, DEV)
    err = lambda got: (R.worst_rel_l2(got[1], want[1]), abs(got[0] - want[0]) / abs(want[0]))  # noqa: E731
    (g_hip, l_hip), (g_32, l_32) = err(hip), err(t32)
    e_hip, e_32 = max(g_hip, l_hip), max(g_32, l_32)
    names = R.param_names(case)
    t_hip, t_32 = R.tensor_errors(hip[1], want[1]), R.tensor_errors(t32[1], want[1])
    core = [n.startswith("nn_module.") for n in names]
    assert any(core) and not all(core)
    nn_hip, nn_32 = (max(e for e, c in zip(t, core) if c) for t in (t_hip, t_32))
    time_hip, time_32 = (max(e for e, c in zip(t, core) if not c) for t in (t_hip, t_32))
    worst = max(zip(t_hip, names))
    print(f"PIS_SHELL_PARITY {R.IDS[k]} {form} e_hip {e_hip:.3e} e_32 {e_32:.3e} (loss {l_hip:.3e} / {l_32:.3e}; "
          f"nn_module {nn_hip:.3e} / {nn_32:.3e}, time networks {time_hip:.3e} / {time_32:.3e}; worst hip tensor "
          f"{worst[1]} {worst[0]:.3e})")
    assert e_hip <= 4 * e_32 and e_hip < 1e-4, (e_hip, e_32, worst)
    assert time_hip <= 4 * time_32, (time_hip, time_32)
    assert nn_hip <= 4 * nn_32, (nn_hip, nn_32)
    tx, y, _ = R.make_batch(k)
    loss, info = _device_objective(case, clip, form)(net, tx.to(DEV), y.to(DEV))
    assert loss.shape == (1,)
    if case[6] > 1e-9:
        assert set(info) == {"train_value_loss", "train_gradient_loss(unscaled)"}
        assert info["train_value_loss"].shape == (1,) and info["train_gradient_loss(unscaled)"].shape == (1,)
    else:
        assert info == {}


def test_adam_trajectory_stays_with_fp64():
    """20 Adam steps (lr 1e-3) on [64] * 4, nx = 10, B = 65 from the same weights on the same batches: the
    objective with the shell in HIP ends no further from the fp64 trajectory than 4 x torch's fp32 objective (the
    bar of tests/test_gpu_pis_fit.py)."""
    k = 2
    case = R.CASES[k]
    assert case[:3] == (65, 10, [64] * 4)
    clip = R.make_batch(k)[2]
    g = torch.Generator().manual_seed(7)
    net64 = R.make_net(case)
    batches = []
    for _ in range(4):
        tx = torch.cat([torch.rand(65, 1, generator=g), torch.randn(65, 10, generator=g)], 1)
        u, u_tx = fit._u_and_grad(net64, tx.double())
        y = torch.cat([u.detach(), u_tx.detach()[:, 1:]], 1) + 0.5 * torch.randn(65, 11, generator=g)
        batches.append((tx, y.float()))

    def run(objective, dtype, device):
        net = R.make_net(case, dtype, device)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        fit.train_steps(net, objective, opt, [(tx.to(dtype=dtype, device=device), y.to(dtype=dtype, device=device))
                                              for tx, y in batches * 5])
        return torch.cat([p.detach().double().cpu().ravel() for p in net.parameters()])

    w64 = run(R.torch_objective(case, clip), torch.float64, "cpu")
    w32 = run(R.torch_objective(case, clip), torch.float32, DEV)
    whip = run(_device_objective(case, clip, "tiles"), torch.float32, DEV)
    d_hip, d_32 = float((whip - w64).norm()), float((w32 - w64).norm())
    print(f"PIS_SHELL_TRAJECTORY distance to fp64 after 20 steps: hip {d_hip:.3e} torch fp32 {d_32:.3e} "
          f"(|w| {float(w64.norm()):.3e})")
    assert d_hip <= 4 * d_32, (d_hip, d_32)


_G = torch.Generator().manual_seed(31)
_MEAN = torch.randn(2, 10, generator=_G).mul(10).round().div(10).tolist()
HJB = """NAME: {name}
EQUATION:
  cls: OUProcessEquation
  kwargs: {{nx: 10, alpha: 1.0, T: 1.0, num_components: 2, alpha_scale: 4.0, mean: {mean},
           var: {var}, pi: [0.4, 0.6]}}
PICARD: {{N: 2}}
FORCE: true
DATA:
  FLOAT: float
  DATA_SIZE: 256
  POINTS_PER_CALL: 128
  EULER_STEPS: 4
  SEED: 11
  kwargs: {{t_always_uniform: true, n_estimate_terminal: 512, n_estimate_integral: 512}}
TRAIN:
  N_EPOCHS: 4
  BATCH_SIZE: 64
  SUPERVISE_GRADIENT: true
  LOSS: {{beta: 0.0, SCALER: {{cls: FixedLossScaler, kwargs: {{fixed_weight: 0.1}}}}}}
  OPTIMIZER: {{kwargs: {{lr: 0.001}}}}
NETWORK:
  cls: PicardSolution
  NEURONS: [64, 64, 64, 64]
  ACTIVATIONS: ["ELU", "ELU", "ELU", "ELU"]
  BOUND: None
  RELOAD: true
  PISGRADNET: true
EVAL: {{L2_N_POINTS: 100, TEST_GRAD: true}}
"""


def test_picard_train_hjb_with_the_shell_in_hip(tmp_path, monkeypatch):
    """`picard train` on the HJB keys at nx = 10, NEURONS [64] * 4, two Picard iterations with TRAIN.BACKEND hip
    TRAIN.PIS_SHELL hip given as overrides, and under the torch backend from the same torch.manual_seed: finite
    checkpoints, fit == "gradient", and iteration 1's first-step losses within 1e-4 relative."""
    first = {}
    steps = runner_module.train_steps

    def recording(net, objective, opt, batches, sched=None):
        losses = steps(net, objective, opt, batches, sched)
        first.setdefault(backend, float(losses[0]))
        return losses

    monkeypatch.setattr(runner_module, "train_steps", recording)
    for backend, override in (("hip", ["TRAIN.BACKEND", "hip", "TRAIN.PIS_SHELL", "hip"]), ("torch", [])):
        f = tmp_path / f"hjb_{backend}.yaml"
        f.write_text(HJB.format(name=tmp_path / f"run_{backend}", mean=_MEAN, var=[[2.0] * 10] * 2))
        torch.manual_seed(123)
        cfg = load_cfg(str(f), override)
        assert cfg.TRAIN.PIS_SHELL == backend
        runner = PicardRunner(cfg)
        runner.run()
        assert [h["iter"] for h in runner.history] == [1, 2]
        lines = [json.loads(l) for l in (tmp_path / f"run_{backend}" / "history.jsonl").read_text().splitlines()]
        assert [l["fit"] for l in lines] == ["gradient"] * 2 and [l["fit_backend"] for l in lines] == [backend] * 2
        for i in (1, 2):
            sd = torch.load(tmp_path / f"run_{backend}" / f"model_{i}.pt", weights_only=True)
            assert all(torch.isfinite(v).all() for v in sd.values())
    print("PIS_SHELL_TRAIN first-step loss of iteration 1", first)
    assert abs(first["hip"] - first["torch"]) <= 1e-4 * abs(first["torch"]), first
