"""The device fit (TRAIN.BACKEND: hip; csrc/dpi_fit.h) on the GPU: parity of its losses
and parameter gradients with torch fp64 autograd of the existing objectives, judged against the error
of today's torch fp32 objective on the same GPU; determinism, canaries and overwrite semantics of the C
call; a 20-step Adam trajectory; and `picard train` end to end under the backend.

Measured on an MI355X over the 30 cases of tests/fit_reference.py: gradients e_hip
4.7e-8 - 1.9e-6 against e_32 9.5e-8 - 1.9e-6 (largest ratio 3.85, a one-element bias gradient), losses
e_hip 2.3e-9 - 8.2e-8 against e_32 2.3e-9 - 1.2e-7; the trajectory distances 1.12e-6 both."""
import ctypes
import json

import numpy as np
import pytest
import torch

import fit_reference as R
from deeppicarditeration_amd import _lib, fit
from deeppicarditeration_amd.config import load_cfg
from deeppicarditeration_amd.runner import PicardRunner

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device_objective(case, clip):
    beta, c, nx = case[4], case[6], case[1]
    loss_fn = torch.square if clip is None else fit.LossFnLinearClip(clip)
    return fit.device_objective(beta, loss_fn, None if c <= 1e-9 else fit.FixedLossScaler(c), nx)


def _device_result(k):
    """losses (2 + nx) and gradients of the device path, through the autograd Function the objective
    is built on (the objective itself reports the per-dimension losses only as their sum)."""
    case = R.CASES[k]
    tx, y, clip = R.make_batch(k)
    net = R.make_net(case, torch.float32, DEV)
    plan = fit._DevicePlan(net, case[1])
    kind = _lib.DPI_FIT_LOSS_SQUARE if clip is None else _lib.DPI_FIT_LOSS_CLIP
    total, parts = fit._DeviceFit.apply(plan, tx.to(DEV), y.to(DEV), case[4], kind, clip or 0.0, case[6], *plan.params)
    total.sum().backward()
    losses = torch.cat([total.detach(), parts]).double().cpu().numpy()
    return losses, [p.grad.double().cpu().numpy() for p in net.parameters()], net


@pytest.mark.parametrize("k", range(len(R.CASES)), ids=R.IDS)
def test_parity_with_fp64_autograd(k):
    """e_hip <= 4 e_32 and e_hip < 1e-4, for the gradients (largest per-tensor rel-L2) and for the loss
    vector: the device path is no further from fp64 than a reordering of torch's own fp32 sums."""
    case = R.CASES[k]
    want_losses, want = R.torch_fp64(k)
    got_losses, got, net = _device_result(k)
    t32_losses, t32 = R.torch_result(k, torch.float32, DEV)
    if case[6] <= 1e-9:  # the value kind forms no gradient losses
        assert not got_losses[2:].any()
    e_hip, e_32 = R.worst_rel_l2(got, want), R.worst_rel_l2(t32, want)
    l_hip, l_32 = R.rel_l2(got_losses, want_losses), R.rel_l2(t32_losses, want_losses)
    print(f"FIT_PARITY {R.IDS[k]} grad e_hip {e_hip:.3e} e_32 {e_32:.3e} loss e_hip {l_hip:.3e} e_32 {l_32:.3e}")
    assert e_hip <= 4 * e_32 and e_hip < 1e-4, (e_hip, e_32)
    assert l_hip <= 4 * l_32 and l_hip < 1e-4, (l_hip, l_32)
    # the objective: the same total, and the info keys of gradient_objective
    tx, y, clip = R.make_batch(k)
    loss, info = _device_objective(case, clip)(net, tx.to(DEV), y.to(DEV))
    assert loss.shape == (1,) and float(loss.detach()) == np.float32(got_losses[0])
    if case[6] > 1e-9:
        assert set(info) == {"train_value_loss", "train_gradient_loss(unscaled)"}
        assert float(info["train_value_loss"]) == np.float32(got_losses[1])
        assert info["train_gradient_loss(unscaled)"].shape == (1,)


CANARY = 4 << 20


def _guarded(nbytes, fill):
    """A tensor of nbytes with a 4 MB canary behind it, from one allocation."""
    buf = torch.full((nbytes + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    if fill is not None:
        buf[:nbytes].view(torch.float32).fill_(fill)
    return buf


@pytest.mark.parametrize("k", [0, 2, 3, 7, 16], ids=[R.IDS[k] for k in (0, 2, 3, 7, 16)])
def test_c_call_is_deterministic_overwrites_and_stays_in_bounds(k):
    """Partial-tile shapes (B = 1, 65, 100): two calls give bit-identical gradients and losses; the
    canaries behind the workspace, `losses` and every gradient tensor are intact; gradients pre-filled
    with NaN come back finite."""
    case = R.CASES[k]
    B, nx, widths = case[0], case[1], case[2]
    tx, y, clip = R.make_batch(k)
    tx, y = tx.to(DEV), y.to(DEV)
    net = R.make_net(case, torch.float32, DEV)
    plan = fit._DevicePlan(net, nx)
    lib = _lib.load()
    need = int(lib.dpi_fit_workspace_bytes(plan.n_in, plan.n_hidden, plan.widths, B))
    runs = []
    for _ in range(2):
        ws = _guarded(need, None)
        losses = _guarded(4 * (2 + nx), float("nan"))
        grads = [_guarded(4 * p.numel(), float("nan")) for p in plan.params]
        tab = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
        _lib.check(lib.dpi_fit_gradients(plan.n_in, plan.n_hidden, plan.widths, plan.act, tab(plan.params[0::2]),
                                         tab(plan.params[1::2]), tab(grads[0::2]), tab(grads[1::2]), tx.data_ptr(),
                                         y.data_ptr(), int(y.stride(0)), B, case[4],
                                         _lib.DPI_FIT_LOSS_SQUARE if clip is None else _lib.DPI_FIT_LOSS_CLIP,
                                         clip or 0.0, case[6], losses.data_ptr(), ws.data_ptr(), need,
                                         torch.cuda.current_stream().cuda_stream), "dpi_fit_gradients")
        torch.cuda.synchronize()
        for buf, n in [(ws, need), (losses, 4 * (2 + nx))] + [(g, 4 * p.numel()) for g, p in zip(grads, plan.params)]:
            assert bool((buf[n:] == 0xA5).all())
        out = [losses[:4 * (2 + nx)].clone()] + [g[:4 * p.numel()].clone() for g, p in zip(grads, plan.params)]
        assert all(bool(torch.isfinite(o.view(torch.float32)).all()) for o in out)
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_adam_trajectory_stays_with_fp64():
    """20 Adam steps (lr 3e-3) on the same batches from the same weights: the device objective ends no
    further from the fp64 trajectory than 4 x today's torch fp32 objective does."""
    k = 2  # B = 65, nx = 7, [32, 32] ELU, beta 0.7, clip, c = 0.1
    case = R.CASES[k]
    _, _, clip = R.make_batch(k)
    g = torch.Generator().manual_seed(7)
    batches = [(torch.cat([torch.rand(65, 1, generator=g), torch.randn(65, 7, generator=g)], 1),
                torch.randn(65, 8, generator=g) * 0.5) for _ in range(4)]

    def run(objective, dtype, device):
        net = R.make_net(case, dtype, device)
        opt = torch.optim.Adam(net.parameters(), lr=3e-3)
        fit.train_steps(net, objective, opt, [(tx.to(dtype=dtype, device=device), y.to(dtype=dtype, device=device))
                                              for tx, y in batches * 5])
        return torch.cat([p.detach().double().cpu().ravel() for p in net.parameters()])

    w64 = run(R.torch_objective(case, clip)[0], torch.float64, "cpu")
    w32 = run(R.torch_objective(case, clip)[0], torch.float32, DEV)
    whip = run(_device_objective(case, clip), torch.float32, DEV)
    d_hip, d_32 = float((whip - w64).norm()), float((w32 - w64).norm())
    print(f"FIT_TRAJECTORY distance to fp64 after 20 steps: hip {d_hip:.3e} torch fp32 {d_32:.3e} "
          f"(|w| {float(w64.norm()):.3e})")
    assert d_hip <= 4 * d_32, (d_hip, d_32)


CHA = """NAME: {name}
EQUATION:
  cls: Cha
  kwargs: {{nx: 8, alpha: 1.0, k: 5.0, T: 1.0}}
PICARD: {{N: 3}}
FORCE: true
DATA:
  DATA_SIZE: 1024
  POINTS_PER_CALL: 384
  EULER_STEPS: 4
  kwargs: {{t_always_uniform: true, n_estimate_terminal: 1024, n_estimate_integral: 1024}}
TRAIN:
  BACKEND: hip
  N_EPOCHS: 16
  BATCH_SIZE: 128
  SUPERVISE_GRADIENT: true
  LOSS: {{beta: 0.0, SCALER: {{cls: FixedLossScaler, kwargs: {{fixed_weight: 0.1}}}}}}
  OPTIMIZER: {{kwargs: {{lr: 0.003}}}}
NETWORK:
  NEURONS: [32, 32]
  ACTIVATIONS: [ELU, ELU]
  BOUND: None
  RELOAD: true
EVAL: {{L2_N_POINTS: 512}}
"""


def test_picard_train_cha_with_the_device_fit(tmp_path):
    f = tmp_path / "cha.yaml"
    f.write_text(CHA.format(name=tmp_path / "run"))
    runner = PicardRunner(load_cfg(str(f)))
    runner.run()
    hist = runner.history
    assert [h["iter"] for h in hist] == [1, 2, 3]
    for i in (1, 2, 3):
        sd = torch.load(tmp_path / "run" / f"model_{i}.pt", weights_only=True)
        assert all(torch.isfinite(v).all() for v in sd.values())
    lines = [json.loads(l) for l in (tmp_path / "run" / "history.jsonl").read_text().splitlines()]
    assert [l["fit"] for l in lines] == ["gradient"] * 3 and [l["fit_backend"] for l in lines] == ["hip"] * 3
    rel = [h["rel_l2_u"] for h in hist]
    print("rel_l2_u per iteration", rel, "fit_s", [h["fit_s"] for h in hist])
    assert max(rel) < 0.6 and min(rel) < 0.3, rel
