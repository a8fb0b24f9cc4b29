"""The device fit of a PISGradNet (TRAIN.BACKEND: hip; the core kernels of csrc/dpi_fit.h)
on the GPU: parity of its loss and of every parameter gradient — nn_module's from the HIP core, the time
networks' through the taubar it returns — with torch fp64 autograd of the existing objectives, judged
against the error of today's torch fp32 objective on the same GPU; determinism, canaries and overwrite
semantics of the C calls; a 20-step Adam trajectory; and `picard train` end to end under the backend.

Measured on an MI355X over the 14 cases of tests/pis_fit_reference.py: e_hip 2.7e-6 - 2.9e-5
against e_32 2.8e-6 - 2.9e-5, e_hip / e_32 0.69 - 1.11; in both the largest error sits in a time network's
tensor (smooth_net, t_encoder), which torch computes under either backend; over nn_module's tensors alone, the
ones the HIP core computes, e_hip is 1.1e-6 - 1.1e-5 against e_32 1.2e-6 - 1.3e-5, ratio 0.64 - 1.11 (the core's
outputs themselves are held to fp64 in tests/test_gpu_pis_core.py).  The trajectory distances are
2.04e-3 (hip) and 2.02e-3 (torch fp32) at |w| = 32; iteration 1's first-step losses of the two backends
were equal to the last bit."""
import ctypes
import json

import pytest
import torch

import pis_fit_reference as R
from deeppicarditeration_amd import _lib, fit, runner as runner_module
from deeppicarditeration_amd.config import load_cfg
from deeppicarditeration_amd.runner import PicardRunner

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device_objective(case, clip):
    beta, c, nx = case[4], case[6], case[1]
    return fit.device_objective(beta, R.loss_fn_of(clip), None if c <= 1e-9 else fit.FixedLossScaler(c), nx)


def _errors(got, want):
    """The largest per-tensor rel-L2 of the gradients, and the loss's relative error."""
    return R.worst_rel_l2(got[1], want[1]), abs(got[0] - want[0]) / abs(want[0])


@pytest.mark.parametrize("k", range(len(R.CASES)), ids=R.IDS)
def test_parity_with_fp64_autograd(k):
    """e_hip <= 4 e_32 and e_hip < 1e-4, e the largest of the per-tensor rel-L2 of all PISGradNet parameter
    gradients and the loss's relative error; and the same factor over the nn_module.* tensors alone."""
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
    worst = max(zip(t_hip, names))
    core = [n.startswith("nn_module.") for n in names]  # the tensors the HIP core computes
    assert any(core) and not all(core)
    nn_hip, nn_32 = (max(e for e, c in zip(t, core) if c) for t in (t_hip, t_32))
    time_hip, time_32 = (max(e for e, c in zip(t, core) if not c) for t in (t_hip, t_32))
    print(f"PIS_FIT_PARITY {R.IDS[k]} e_hip {e_hip:.3e} e_32 {e_32:.3e} (grad {g_hip:.3e} / {g_32:.3e}, loss "
          f"{l_hip:.3e} / {l_32:.3e}; nn_module {nn_hip:.3e} / {nn_32:.3e}, time networks {time_hip:.3e} / "
          f"{time_32:.3e}; worst hip tensor {worst[1]} {worst[0]:.3e})")
    assert e_hip <= 4 * e_32 and e_hip < 1e-4, (e_hip, e_32, worst)
    # the same bound on the core's own tensors: the time networks' larger error does not cover for them
    assert nn_hip <= 4 * nn_32, (nn_hip, nn_32)
    # the objective's contract: gradient_objective's info keys; the value kind returns {}
    tx, y, _ = R.make_batch(k)
    loss, info = _device_objective(case, clip)(net, tx.to(DEV), y.to(DEV))
    assert loss.shape == (1,)
    if case[6] > 1e-9:
        assert set(info) == {"train_value_loss", "train_gradient_loss(unscaled)"}
        assert info["train_value_loss"].shape == (1,) and info["train_gradient_loss(unscaled)"].shape == (1,)
    else:
        assert info == {}


def test_value_kind_forms_no_q():
    k = next(k for k, c in enumerate(R.CASES) if c[6] <= 1e-9)
    case = R.CASES[k]
    net = R.make_net(case, torch.float32, DEV)
    plan = fit._PISPlan(net, case[1])
    tx = R.make_batch(k)[0].to(DEV)
    tau = torch.randn(case[0], 64, device=DEV)
    sp, q = fit._PISCore.apply(plan, False, tau, tx[:, 1:], *plan.params)
    assert sp.shape == (case[0], 1) and q.numel() == 0 and bool(torch.isfinite(sp).all())


CANARY = 4 << 20


def _guarded(nbytes, fill):
    """A tensor of nbytes with a 4 MB canary behind it, from one allocation."""
    buf = torch.full((nbytes + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    if fill is not None:
        buf[:nbytes].view(torch.float32).fill_(fill)
    return buf


PARTIAL = [k for k, c in enumerate(R.CASES) if c[0] in (1, 65, 100) and c[6] > 1e-9]


@pytest.mark.parametrize("k", PARTIAL, ids=[R.IDS[k] for k in PARTIAL])
def test_c_calls_are_deterministic_overwrite_and_stay_in_bounds(k):
    """Partial-tile shapes (B = 1, 65, 100): two forward + backward calls give bit-identical sp, q, taubar
    and gradients; the canaries behind the workspace and every output are intact; outputs pre-filled with
    NaN come back finite."""
    case = R.CASES[k]
    B, nx = case[0], case[1]
    net = R.make_net(case, torch.float32, DEV)
    plan = fit._PISPlan(net, nx)
    lib = _lib.load()
    g = torch.Generator().manual_seed(5000 + k)
    tau, x, e, r = (torch.randn(B, n, generator=g).to(DEV) for n in (64, nx, 1, nx))
    need = int(lib.dpi_fit_core_workspace_bytes(nx, plan.n_hidden, plan.widths, B))
    assert need > 0
    st = torch.cuda.current_stream().cuda_stream
    tab = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    runs = []
    for _ in range(2):
        ws = _guarded(need, None)
        sizes = [4 * B, 4 * B * nx, 4 * B * 64] + [4 * p.numel() for p in plan.params]
        sp, q, dtau, *grads = [_guarded(n, float("nan")) for n in sizes]
        _lib.check(lib.dpi_fit_core_forward(nx, plan.n_hidden, plan.widths, tab(plan.params[0::2]),
                                            tab(plan.params[1::2]), tau.data_ptr(), 64, x.data_ptr(), nx, B,
                                            sp.data_ptr(), q.data_ptr(), ws.data_ptr(), need, st), "forward")
        _lib.check(lib.dpi_fit_core_backward(nx, plan.n_hidden, plan.widths, tab(plan.params[0::2]),
                                             tab(plan.params[1::2]), tab(grads[0::2]), tab(grads[1::2]), e.data_ptr(),
                                             r.data_ptr(), B, dtau.data_ptr(), ws.data_ptr(), need, st), "backward")
        torch.cuda.synchronize()
        bufs = [sp, q, dtau, *grads]
        for buf, n in [(ws, need)] + list(zip(bufs, sizes)):
            assert bool((buf[n:] == 0xA5).all())
        out = [b[:n].clone() for b, n in zip(bufs, sizes)]
        assert all(bool(torch.isfinite(o.view(torch.float32)).all()) for o in out)
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_adam_trajectory_stays_with_fp64():
    """20 Adam steps (lr 1e-3) on [64] * 4, nx = 10, B = 65 from the same weights on the same batches: the
    device objective ends no further from the fp64 trajectory than 4 x today's torch fp32 objective."""
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
    whip = run(_device_objective(case, clip), torch.float32, DEV)
    d_hip, d_32 = float((whip - w64).norm()), float((w32 - w64).norm())
    print(f"PIS_FIT_TRAJECTORY distance to fp64 after 20 steps: hip {d_hip:.3e} torch fp32 {d_32:.3e} "
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
  BACKEND: {backend}
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


def test_picard_train_hjb_with_the_device_fit(tmp_path, monkeypatch):
    """`picard train` on the HJB keys of tests/test_gpu_train.py at nx = 10, NEURONS [64] * 4, two Picard
    iterations under each backend from the same torch.manual_seed: same labels (Philox) and same initial
    weights, so iteration 1's first-step losses agree to 1e-4 relative."""
    first = {}
    steps = runner_module.train_steps

    def recording(net, objective, opt, batches, sched=None):
        losses = steps(net, objective, opt, batches, sched)
        first.setdefault(backend, float(losses[0]))
        return losses

    monkeypatch.setattr(runner_module, "train_steps", recording)
    for backend in ("hip", "torch"):
        f = tmp_path / f"hjb_{backend}.yaml"
        f.write_text(HJB.format(name=tmp_path / f"run_{backend}", backend=backend, mean=_MEAN, var=[[2.0] * 10] * 2))
        torch.manual_seed(123)
        runner = PicardRunner(load_cfg(str(f)))
        runner.run()
        assert [h["iter"] for h in runner.history] == [1, 2]
        lines = [json.loads(l) for l in (tmp_path / f"run_{backend}" / "history.jsonl").read_text().splitlines()]
        assert [l["fit"] for l in lines] == ["gradient"] * 2 and [l["fit_backend"] for l in lines] == [backend] * 2
        for i in (1, 2):
            sd = torch.load(tmp_path / f"run_{backend}" / f"model_{i}.pt", weights_only=True)
            assert all(torch.isfinite(v).all() for v in sd.values())
    print("PIS_FIT_TRAIN first-step loss of iteration 1", first)
    assert abs(first["hip"] - first["torch"]) <= 1e-4 * abs(first["torch"]), first
