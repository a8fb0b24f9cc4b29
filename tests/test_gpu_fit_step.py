"""The fused training step (TRAIN.FUSED_STEP; dpi_fit_step, k_fit_wgrad_step) on the GPU: its
losses and gradients are dpi_fit_gradients' to the bit; one update against the fp64 restatement of torch's
Adam / AdamW (tests/adam_reference.py), judged against torch's own fp32 single-tensor update of the same
gradients on the same GPU; a 20-step trajectory; canaries behind everything the call may write; determinism;
and `picard train` end to end with the key on and off.

Measured on an MI355X: one update, over the 10 cases x 8 (optimizer, weight decay, step)
settings, e_hip up to 3.8e-7 (w), 1.4e-7 (exp_avg), 1.5e-7 (exp_avg_sq) against e_32 up to 6.8e-7, 6.3e-8,
1.5e-7 and the floor 2^-24 = 6.0e-8; largest e_hip / max(e_32, 2^-24) 3.52 (the one-element output bias at
B = 1, [24] * 8), 2.19 for a weight matrix; trajectory distances to fp64 after 20 steps: fused 1.093e-6,
device objective + torch Adam 1.077e-6."""
import ctypes
import json

import pytest
import torch

import adam_reference as A
import fit_reference as R
from deeppicarditeration_amd import _lib, fit
from deeppicarditeration_amd.config import load_cfg
from deeppicarditeration_amd.runner import PicardRunner
from deeppicarditeration_amd.solution import construct_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLIP = 0.4  # labels are 0.5 randn: residuals fall on both branches of LossFnLinearClip

# (B, nx, hidden widths, activation, beta, clipped, c, y row stride beyond 1 + nx): the smallest shapes where
# the tiles, the row walk and the tables can go wrong.  B: one row (the odd tail of a chunk), a second tile
# with one live row, a partly filled second tile.  Nets: one weight tile; nin = 8 < 16 and nout = 129 (a
# one-row tile); the deepest blk0 table; the widest tables (once).  c = 0 is the value kind (a.grad == 0).
NETS = [([16], "ELU", 7), ([129], "Tanh", 7), ([24] * 8, "Tanh", 7)]
CASES = [(B, nx, w, act, beta, clipped, c, extra)
         for (w, act, nx), opts in zip(NETS, [[(0.0, False, 1.0, 0), (0.7, True, 0.1, 0), (0.0, False, 0.0, 0)],
                                              [(0.7, True, 0.0, 0), (0.0, False, 1.0, 49), (0.7, True, 0.1, 0)],
                                              [(0.7, False, 0.1, 0), (0.0, True, 0.0, 0), (0.7, True, 1.0, 0)]])
         for B, (beta, clipped, c, extra) in zip((1, 65, 100), opts)]
CASES.append((65, 100, [256] * 2, "ELU", 0.7, False, 1.0, 0))
IDS = [f"B{c[0]}-nx{c[1]}-{len(c[2])}x{max(c[2])}-{c[3]}-b{c[4]}-{'clip' if c[5] else 'sq'}-c{c[6]}"
       + ("-wide_y" if c[7] else "") for c in CASES]
SETTINGS = [(cls, wd, step) for cls in ("Adam", "AdamW") for wd in (0.0, 0.01) for step in (1, 1000)]
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)


def _setup(case, seed=0):
    """The case's network (fit_reference's gain on the hidden weights), plan, batch on the device and loss
    arguments."""
    B, nx, widths, act, beta, clipped, c, extra = case
    torch.manual_seed(3000 + seed)
    net = construct_mlp(1 + nx, 1, list(widths), [act] * len(widths), None)
    with torch.no_grad():
        for m in list(net)[:-1]:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(R.GAIN)
    net = net.to(DEV)
    g = torch.Generator().manual_seed(4000 + seed)
    tx = torch.cat([torch.rand(B, 1, generator=g), torch.randn(B, nx, generator=g)], 1).to(DEV)
    y = (torch.randn(B, 1 + nx + extra, generator=g) * 0.5).to(DEV)
    kind = _lib.DPI_FIT_LOSS_CLIP if clipped else _lib.DPI_FIT_LOSS_SQUARE
    return net, fit._DevicePlan(net, nx), tx, y, (beta, kind, CLIP if clipped else 0.0, c)


def _moments(params, seed):
    """Moments that are not zero: exp_avg random, exp_avg_sq random and non-negative, at the gradients' size."""
    g = torch.Generator().manual_seed(5000 + seed)
    m = [(torch.randn(p.shape, generator=g) * 1e-2).to(DEV) for p in params]
    v = [(torch.rand(p.shape, generator=g) * 1e-4).to(DEV) for p in params]
    return m, v


def _tab(ts):
    return None if ts is None else (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _ws(plan, B):
    need = int(_lib.load().dpi_fit_workspace_bytes(plan.n_in, plan.n_hidden, plan.widths, B))
    return torch.empty(need, dtype=torch.uint8, device=DEV), need


def _gradients(plan, params, tx, y, loss):
    lib = _lib.load()
    ws, need = _ws(plan, tx.shape[0])
    grads = [torch.full_like(p, float("nan")) for p in params]
    losses = torch.full((1 + plan.n_in,), float("nan"), device=DEV)
    beta, kind, clip, c = loss
    _lib.check(lib.dpi_fit_gradients(plan.n_in, plan.n_hidden, plan.widths, plan.act, _tab(params[0::2]),
                                     _tab(params[1::2]), _tab(grads[0::2]), _tab(grads[1::2]), tx.data_ptr(),
                                     y.data_ptr(), int(y.stride(0)), tx.shape[0], beta, kind, clip, c, losses.data_ptr(),
                                     ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "dpi_fit_gradients")
    return losses, grads


def _step(plan, params, m, v, tx, y, loss, grads=None, losses=None, ws=None, cls="Adam", wd=0.0, step=1, **hyper):
    """dpi_fit_step on (params, m, v) in place; returns losses."""
    lib = _lib.load()
    hyper = {**HYPER, **hyper}
    if ws is None:
        ws = _ws(plan, tx.shape[0])
    if losses is None:
        losses = torch.full((1 + plan.n_in,), float("nan"), device=DEV)
    beta, kind, clip, c = loss
    _lib.check(lib.dpi_fit_step(plan.n_in, plan.n_hidden, plan.widths, plan.act, _tab(params[0::2]), _tab(params[1::2]),
                                _tab(grads and grads[0::2]), _tab(grads and grads[1::2]), _tab(m[0::2]), _tab(m[1::2]),
                                _tab(v[0::2]), _tab(v[1::2]), tx.data_ptr(), y.data_ptr(), int(y.stride(0)), tx.shape[0],
                                beta, kind, clip, c, hyper["lr"], *hyper["betas"], hyper["eps"], wd, int(cls == "AdamW"),
                                step, losses.data_ptr(), ws[0].data_ptr(), ws[1],
                                torch.cuda.current_stream().cuda_stream), "dpi_fit_step")
    return losses


def _clone(ts):
    return [t.detach().clone() for t in ts]


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_gradients_and_losses_are_the_gradient_calls(k):
    """With gradient tables on a copy of the weights: losses, dW and db torch.equal to dpi_fit_gradients; a
    second call with NULL tables leaves weights and moments bit-identical to the first."""
    net, plan, tx, y, loss = _setup(CASES[k], k)
    want_losses, want = _gradients(plan, plan.params, tx, y, loss)
    m0, v0 = _moments(plan.params, k)
    runs = []
    for with_tables in (True, False):
        w, m, v = _clone(plan.params), _clone(m0), _clone(v0)
        grads = [torch.full_like(p, float("nan")) for p in w] if with_tables else None
        losses = _step(plan, w, m, v, tx, y, loss, grads=grads, cls="AdamW", wd=0.01, step=3)
        assert torch.equal(losses, want_losses)
        if with_tables:
            assert all(torch.equal(g, h) for g, h in zip(grads, want))
        assert all(not torch.equal(a, p) for a, p in zip(w, plan.params))  # every tensor was stepped
        runs.append(w + m + v)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    if CASES[k][6] <= 1e-9:  # the value kind forms no gradient losses
        assert not want_losses[2:].any()


def _rel(got, want):
    return R.rel_l2(got.double().cpu().numpy(), want)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_one_step_against_fp64(k):
    """From moments that are not zero, at step 1 and 1000, Adam and AdamW, weight decay 0 and 0.01: for w,
    exp_avg and exp_avg_sq of every tensor, the rel-L2 against the fp64 reference applied to the fp32
    gradients is within 4 x max(e_32, 2^-24), e_32 that of torch's own fp32 update (foreach=False) fed the
    same gradients on the same GPU and 2^-24 the fp32 half-ulp."""
    net, plan, tx, y, loss = _setup(CASES[k], k)
    _, grads = _gradients(plan, plan.params, tx, y, loss)
    m0, v0 = _moments(plan.params, k)
    f64 = lambda ts: [t.detach().double().cpu().numpy() for t in ts]  # noqa: E731
    worst = 0.0
    for cls, wd, step in SETTINGS:
        truth = A.adam_steps(f64(plan.params), f64(m0), f64(v0), f64(grads), step, weight_decay=wd,
                             decoupled=cls == "AdamW", **HYPER)
        w, m, v = _clone(plan.params), _clone(m0), _clone(v0)
        _step(plan, w, m, v, tx, y, loss, cls=cls, wd=wd, step=step)
        ps = [torch.nn.Parameter(p.detach().clone()) for p in plan.params]
        opt = getattr(torch.optim, cls)(ps, weight_decay=wd, foreach=False, **HYPER)
        for p, g, a, b in zip(ps, grads, m0, v0):
            p.grad = g.clone()
            opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": a.clone(), "exp_avg_sq": b.clone()}
        opt.step()
        t32 = ([p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps])
        for name, got, ref, want in zip(("w", "exp_avg", "exp_avg_sq"), (w, m, v), t32, truth):
            for i, (a, b, t) in enumerate(zip(got, ref, want)):
                e_hip, e_32 = _rel(a, t), _rel(b, t)
                worst = max(worst, e_hip / max(e_32, 2.0 ** -24))
                print(f"FIT_STEP {IDS[k]} {cls} wd {wd} step {step} {name}[{i}] e_hip {e_hip:.3e} e_32 {e_32:.3e}")
                assert e_hip <= 4 * max(e_32, 2.0 ** -24), (cls, wd, step, name, i, e_hip, e_32)
    print(f"FIT_STEP_WORST {IDS[k]} e_hip / max(e_32, 2^-24) = {worst:.3f}")


def test_trajectory_stays_with_fp64():
    """20 steps at lr 3e-3 on the same batches from the same weights ([32, 32] ELU, nx = 8, B = 65, c = 0.1):
    the fused step ends no further from the fp64 CPU trajectory than 4 x today's path (device objective plus
    torch Adam) does."""
    g = torch.Generator().manual_seed(7)
    batches = [(torch.cat([torch.rand(65, 1, generator=g), torch.randn(65, 8, generator=g)], 1),
                torch.randn(65, 9, generator=g) * 0.5) for _ in range(4)] * 5
    scaler = fit.FixedLossScaler(0.1)

    def run(form, dtype, device):
        torch.manual_seed(1234)
        net = construct_mlp(9, 1, [32, 32], ["ELU", "ELU"], None)
        with torch.no_grad():
            net[0].weight.mul_(R.GAIN), net[2].weight.mul_(R.GAIN)
        net = net.to(dtype=dtype, device=device)
        opt = torch.optim.Adam(net.parameters(), lr=3e-3)
        data = [(tx.to(dtype=dtype, device=device), y.to(dtype=dtype, device=device)) for tx, y in batches]
        if form == "fused":
            losses = fit.fused_train_steps(net, fit.device_step(0.3, torch.square, scaler, 8), opt, data)
            assert all(p.grad is None for p in net.parameters())
            assert all(float(opt.state[p]["step"]) == 20 for p in net.parameters())
        else:
            objective = (fit.device_objective if form == "device" else fit.gradient_objective)(0.3, torch.square,
                                                                                             scaler, 8)
            losses = fit.train_steps(net, objective, opt, data)
        assert losses.shape == (20,) and bool(torch.isfinite(losses).all())
        return torch.cat([p.detach().double().cpu().ravel() for p in net.parameters()])

    w64 = run("torch", torch.float64, "cpu")
    d_fused = float((run("fused", torch.float32, DEV) - w64).norm())
    d_unfused = float((run("device", torch.float32, DEV) - w64).norm())
    print(f"FIT_STEP_TRAJECTORY distance to fp64 after 20 steps: fused {d_fused:.3e} unfused {d_unfused:.3e} "
          f"(|w| {float(w64.norm()):.3e})")
    assert d_fused <= 4 * d_unfused, (d_fused, d_unfused)


CANARY = 4 << 20


def _guarded(src):
    """A copy of fp32 tensor `src` with a 4 MB canary behind it, from one allocation: (buffer, the copy)."""
    n = 4 * src.numel()
    buf = torch.full((n + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    view = buf[:n].view(torch.float32).view(src.shape)
    view.copy_(src)
    return buf, view


@pytest.mark.parametrize("k", [3, 4, 5], ids=[IDS[k] for k in (3, 4, 5)])
@pytest.mark.parametrize("tables", [True, False], ids=["grads", "no_grads"])
def test_nothing_else_is_written(k, tables):
    """[129] at B = 1, 65, 100: the 4 MB canaries behind the workspace, `losses`, every weight, bias and moment
    tensor and, when present, every gradient tensor are intact; NaN-prefilled gradients and losses come back
    finite."""
    net, plan, tx, y, loss = _setup(CASES[k], k)
    m0, v0 = _moments(plan.params, k)
    need = _ws(plan, tx.shape[0])[1]
    ws = torch.full((need + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    nan = lambda p: torch.full_like(p, float("nan"))  # noqa: E731
    groups = [[_guarded(t) for t in ts] for ts in (plan.params, m0, v0)]
    gbufs = [_guarded(nan(p)) for p in plan.params] if tables else None
    lbuf, losses = _guarded(torch.full((1 + plan.n_in,), float("nan"), device=DEV))
    w, m, v = ([view for _, view in grp] for grp in groups)
    _step(plan, w, m, v, tx, y, loss, grads=[view for _, view in gbufs] if tables else None, losses=losses,
          ws=(ws, need), cls="Adam", wd=0.01, step=2)
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all())
    for buf, view in [(lbuf, losses)] + [bv for grp in groups for bv in grp] + (gbufs or []):
        assert bool((buf[4 * view.numel():] == 0xA5).all())
        assert bool(torch.isfinite(view).all())


def test_determinism():
    """Two runs of 3 steps from cloned state: bit-identical weights, moments and losses."""
    k = 5
    net, plan, tx, y, loss = _setup(CASES[k], k)
    m0, v0 = _moments(plan.params, k)
    runs = []
    for _ in range(2):
        w, m, v = _clone(plan.params), _clone(m0), _clone(v0)
        out = [_step(plan, w, m, v, tx, y, loss, cls="AdamW", wd=0.01, step=s) for s in (1, 2, 3)]
        runs.append(out + w + m + v)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], runs[0][2])  # the steps moved the loss


CHA = """NAME: {name}
EQUATION:
  cls: Cha
  kwargs: {{nx: 8, alpha: 1.0, k: 5.0, T: 1.0}}
PICARD: {{N: 2}}
FORCE: true
DATA:
  DATA_SIZE: 512
  POINTS_PER_CALL: 256
  EULER_STEPS: 4
  kwargs: {{t_always_uniform: true, n_estimate_terminal: 256, n_estimate_integral: 256}}
TRAIN:
  BACKEND: hip
  FUSED_STEP: {fused}
  N_EPOCHS: 4
  BATCH_SIZE: 128
  SUPERVISE_GRADIENT: true
  LOSS: {{beta: 0.0, SCALER: {{cls: FixedLossScaler, kwargs: {{fixed_weight: 0.1}}}}}}
  OPTIMIZER: {{kwargs: {{lr: 0.003}}}}
NETWORK:
  NEURONS: [32, 32]
  ACTIVATIONS: [ELU, ELU]
  BOUND: None
  RELOAD: true
EVAL: {{L2_N_POINTS: 256}}
"""


def test_picard_train_with_the_key_on_and_off(tmp_path):
    first = {}
    for fused in (True, False):
        f = tmp_path / f"cha_{fused}.yaml"
        f.write_text(CHA.format(name=tmp_path / f"run_{fused}", fused=str(fused).lower()))
        torch.manual_seed(99)  # the same initial weights; the labels are seeded by DATA.SEED
        runner = PicardRunner(load_cfg(str(f)))
        runner.run_one()
        first[fused] = runner.fit_losses.detach().cpu()
        runner.run_one()
        lines = [json.loads(l) for l in (tmp_path / f"run_{fused}" / "history.jsonl").read_text().splitlines()]
        assert [l["iter"] for l in lines] == [1, 2] and [l["fit_backend"] for l in lines] == ["hip"] * 2
        assert [l["fit_step"] for l in lines] == ["fused" if fused else "torch"] * 2
        assert [l["fit"] for l in lines] == ["gradient"] * 2
        for i in (1, 2):
            sd = torch.load(tmp_path / f"run_{fused}" / f"model_{i}.pt", weights_only=True)
            assert all(torch.isfinite(v).all() for v in sd.values())
    a, b = first[True], first[False]
    print("first 8 per-step losses of iteration 1: fused", a[:8].tolist(), "torch", b[:8].tolist())
    assert a.shape == b.shape == (16,)
    assert a[0] == b[0]  # formed before the update, from the same labels and weights: equal to the last bit
    assert torch.allclose(a[:8], b[:8], rtol=1e-4, atol=0)
