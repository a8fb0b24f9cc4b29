"""The device fit of a PISGradNet restated in numpy fp64 ("The PISGradNet core"): the
four passes of the core primitive (tau, x, nn_module's parameters) -> (sp, q = d sp / d x) and their
backward, the objective around them, the case table the CPU and GPU tests share, and the torch side of
the comparison (fit.gradient_objective / fit.value_objective on the whole PISGradNet under autograd).
For the core alone: its own case table and call forms (CORE_CASES, MODES, core_case), the restatement's direct
outputs in fp64 or fp32 (core_outputs; the passes run in the dtype of their inputs) and torch autograd of the
same primitive (torch_core).  No GPU and no library is needed to import this module."""
import functools

import numpy as np
import torch

from deeppicarditeration_amd import fit
from deeppicarditeration_amd.equations import OUProcessEquation
from deeppicarditeration_amd.solution import PISGradNet

NT = 64  # tau columns (PISGradNet.channels)

# (B, nx, hidden widths of nn_module, T, beta, clip?, c)
# B: 1, a whole 64-row tile, one row past it, a partial second tile, 8 tiles.  Nets: one layer, the nest
# YAML's [64] * 4, widths that are no multiple of the unit block or the weight tile ([130, 70]), [512] * 2 and
# the HJB YAML's [512] * 4 once at B = 64.  c = 0 is the value kind (only sp is formed).  c reaches torch's
# loss only, never the kernels; at nx >= 100 it is 1, since with 0.1 the whole of pass 3 is 4e-4 - 6e-4 of the
# gradient there, below what the gates ask a mutant to move.
CASES = [
    (1, 3, [16], 1.0, 0.0, False, 1.0),
    (64, 10, [64] * 4, 1.0, 0.7, False, 1.0),
    (65, 10, [64] * 4, 1.0, 0.7, True, 0.1),
    (100, 3, [130, 70], 1.0, 0.0, True, 1.0),
    (512, 10, [64] * 4, 1.0, 0.7, False, 1.0),
    (100, 100, [130, 70], 0.5, 0.7, False, 1.0),
    (65, 128, [16], 1.0, 0.0, True, 1.0),
    (512, 100, [512] * 2, 1.0, 0.0, False, 1.0),
    (64, 100, [512] * 4, 1.0, 0.7, False, 1.0),
    (100, 10, [64] * 4, 1.0, 0.7, True, 0.0),
    (65, 3, [130, 70], 1.0, 0.0, False, 0.0),
    (1, 128, [130, 70], 1.0, 0.7, False, 1.0),
    (1, 10, [64] * 4, 1.0, 0.0, True, 0.1),
    (100, 128, [16], 1.0, 0.7, False, 1.0),
]
IDS = [f"{k}-B{c[0]}-nx{c[1]}-{len(c[2])}x{max(c[2])}-T{c[3]}-b{c[4]}-{'clip' if c[5] else 'sq'}-c{c[6]}"
       for k, c in enumerate(CASES)]
NOISE = 0.3  # the labels' distance from the network's own outputs, relative to their rms (make_batch)
MUTANTS = ("no_tangent", "no_N", "no_v_lambdabar", "no_dtau")
# mutants of the core alone, each one edge of the kernels (tests/test_pis_core_reference.py): the remainder loop
# of fit_mv / fit_mvT, k_fit_core_wgrad's unpaired last row, and phi'' on the linear branch of ELU
CORE_MUTANTS = ("tail_k", "odd_row", "elu2_everywhere")

# The core alone, (B, nx, hidden widths): the shapes at which k_fit_core_fwd / _bwd / _wgrad take another branch
# or reach a bound.  n0 = 64 + nx is the first layer's row count.
CORE_CASES = [
    (1, 3, [16]),              # one row; n0 = 67
    (65, 1, [3]),              # nx = 1; a width below the 4-unit block; a second tile with one live row
    (1, 128, [1]),             # width 1 at the nx cap
    (65, 10, [64] * 4),        # the nest YAML's network
    (100, 3, [130, 70]),       # no multiple of 4 or 16
    (129, 127, [17, 511]),     # three tiles, the last with one live row; odd nx, n0 = 191; one unit past a weight
                               # tile; one under the width cap
    (64, 128, [512] * 4),      # every cap at once: the LDS vector is full
    (100, 128, [16]),          # a wide input into one weight-tile row
    (512, 10, [64] * 2),       # eight tiles
]
CORE_IDS = [f"{k}-B{c[0]}-nx{c[1]}-{'x'.join(map(str, c[2]))}" for k, c in enumerate(CORE_CASES)]
# grad: q formed, e and r given.  value: q NULL, r NULL.  sp_cot_only: q formed, r NULL in the backward.
# q_cot_only: q formed, e = 0.
MODES = ("grad", "value", "sp_cot_only", "q_cot_only")


def _elu(z):
    """phi, phi', phi'' of ELU (alpha = 1), in z's dtype."""
    e = np.exp(np.minimum(z, 0))
    one, zero = z.dtype.type(1), z.dtype.type(0)
    return np.where(z > 0, z, e - one), np.where(z > 0, one, e), np.where(z > 0, zero, e)


def _mm(a, b, mutant):
    """a (B, K) @ b (K, N); under tail_k the last K % 4 terms of every sum are dropped (the remainder loop of
    fit_mv / fit_mvT)."""
    if mutant == "tail_k":
        k = a.shape[1] - a.shape[1] % 4
        return a[:, :k] @ b[:k]
    return a @ b


def core_forward(Ws, bs, tau, x, grad=True, mutant=None):
    """Passes 1 and 2, in the dtype of the inputs.  Ws, bs: nn_module's L + 1 layers, (out, in) and (out,);
    tau (B, 64), x (B, nx).  Returns sp (B, 1), q (B, nx) or None, and the state the backward needs."""
    L = len(Ws) - 1
    a, d1, d2 = [np.concatenate([tau, x], axis=1)], [None], [None]
    for l in range(L):  # 1. forward
        f, g, h = _elu(_mm(a[-1], Ws[l].T, mutant) + bs[l])
        if mutant == "elu2_everywhere":
            h = g
        a.append(f), d1.append(g), d2.append(h)
    N = _mm(a[L], Ws[L].T, mutant) + bs[L]
    sp = np.sum(x * N, axis=1, keepdims=True)
    st = {"a": a, "d1": d1, "d2": d2, "x": x}
    if not grad:
        return sp, None, st
    lam, delta = [None] * (L + 1), [None] * (L + 1)  # 2. adjoint, delta_{L+1} = v = x
    lam[L] = _mm(x, Ws[L], mutant)
    for l in range(L, 0, -1):
        delta[l] = lam[l] * d1[l]
        lam[l - 1] = _mm(delta[l], Ws[l - 1], mutant)
    q = lam[0][:, NT:] + (0 if mutant == "no_N" else N)
    st.update(lam=lam, delta=delta)
    return sp, q, st


def core_backward(Ws, st, e, r, mutant=None):
    """Passes 3 and 4 from the cotangents e (B, 1) of sp and r (B, nx) of q (None: q was not formed, or has
    no cotangent), in the dtype of the state.  Returns dWs, dbs and taubar (B, 64)."""
    L = len(Ws) - 1
    a, d1, d2, x = st["a"], st["d1"], st["d2"], st["x"]
    B = x.shape[0]
    rows = slice(0, B - 1) if mutant == "odd_row" and B % 2 else slice(0, B)  # the batch rows dW and db sum
    dWs = [np.zeros_like(W) for W in Ws]
    dbs = [None] * (L + 1)
    zeta = [None] * (L + 1)
    if r is not None and mutant != "no_tangent":  # 3. tangent of the adjoint chain, lambdabar_0 = (0_tau, r)
        lam, delta = st["lam"], st["delta"]
        lb = np.concatenate([np.zeros((B, NT), dtype=r.dtype), r], axis=1)
        for l in range(1, L + 1):
            db_ = _mm(lb, Ws[l - 1].T, mutant)
            dWs[l - 1] += delta[l][rows].T @ lb[rows]
            lb = db_ * d1[l]
            zeta[l] = db_ * lam[l] * d2[l]
        if mutant != "no_v_lambdabar":
            dWs[L] += x[rows].T @ lb[rows]
    zb = e * x + (0 if r is None else r)  # 4. reverse, zbar_{L+1} = e v + r, down to abar_0
    dWs[L] += zb[rows].T @ a[L][rows]
    dbs[L] = zb[rows].sum(axis=0)
    abar = _mm(zb, Ws[L], mutant)
    for l in range(L, 0, -1):
        zb = abar * d1[l] + (0 if zeta[l] is None else zeta[l])
        dWs[l - 1] += zb[rows].T @ a[l - 1][rows]
        dbs[l - 1] = zb[rows].sum(axis=0)
        abar = _mm(zb, Ws[l - 1], mutant)
    taubar = abar[:, :NT] * (0 if mutant == "no_dtau" else 1)
    return dWs, dbs, taubar


def core_case(k, mode, seed=0):
    """fp32 numpy (Ws, bs, tau, x, e, r) of CORE_CASES[k]: W = (U(-1, 1) + N(0, 1)) / sqrt(fan_in), b =
    U(-1, 1) / sqrt(fan_in) + 0.3 N(0, 1), tau, x, e, r standard normals, drawn in the order returned (every
    W, the uniform part first; then every b; then the data) whatever the mode, so the modes of a case share
    their inputs.  r is None where the backward gets none (value, sp_cot_only) and e is zeros under
    q_cot_only.  The cap of tests/test_pis_core_reference.py (E_case <= 2e-6) is a condition on these very
    draws: at B = 1, sp is one number, x . N, and a draw in which its nx terms cancel would fail the cap
    before any kernel is looked at.  Change the draws and the cap has to be checked again."""
    assert mode in MODES
    B, nx, widths = CORE_CASES[k]
    rng = np.random.default_rng(100 + k + 1000 * seed)
    n = [NT + nx] + list(widths) + [nx]
    fan = list(zip(n[1:], n[:-1]))
    Ws = [((rng.uniform(-1, 1, (o, i)) + rng.standard_normal((o, i))) * i ** -0.5).astype(np.float32) for o, i in fan]
    bs = [(rng.uniform(-1, 1, o) * i ** -0.5 + 0.3 * rng.standard_normal(o)).astype(np.float32) for o, i in fan]
    tau, x, e, r = (rng.standard_normal((B, m)).astype(np.float32) for m in (NT, nx, 1, nx))
    if mode == "q_cot_only":
        e = np.zeros_like(e)
    if mode in ("value", "sp_cot_only"):
        r = None
    return Ws, bs, tau, x, e, r


def core_names(k):
    """The core's outputs in the order core_outputs and torch_core return them."""
    L1 = len(CORE_CASES[k][2]) + 1
    return ["sp", "q", "dtau"] + [f"dW{l}" for l in range(1, L1 + 1)] + [f"db{l}" for l in range(1, L1 + 1)]


def core_outputs(inputs, mode, dtype=np.float64, mutant=None):
    """[sp, q or None, taubar, dW_1 .., db_1 ..] of the restatement run in `dtype` on the inputs of core_case."""
    Ws, bs, tau, x, e, r = [[a.astype(dtype) for a in v] if isinstance(v, list) else
                            (None if v is None else v.astype(dtype)) for v in inputs]
    sp, q, st = core_forward(Ws, bs, tau, x, grad=mode != "value", mutant=mutant)
    dWs, dbs, taubar = core_backward(Ws, st, e, r, mutant=mutant)
    out = [sp, q, taubar] + dWs + dbs
    assert all(o is None or o.dtype == dtype for o in out)
    return out


def torch_core(inputs, mode, dtype=torch.float64, device="cpu"):
    """The same outputs from torch autograd: nn_module rebuilt from Ws and bs, sp = (x N).sum(1), q =
    grad(sp.sum(), x, create_graph=True), and the cotangent (e sp).sum() + (r q).sum().  fp64 numpy."""
    t = lambda a: None if a is None else torch.from_numpy(a).to(dtype=dtype, device=device)  # noqa: E731
    Ws, bs = [t(W).requires_grad_() for W in inputs[0]], [t(b).requires_grad_() for b in inputs[1]]
    tau, x, e, r = (t(a) for a in inputs[2:])
    tau.requires_grad_(), x.requires_grad_()
    h = torch.cat([tau, x], 1)
    for W, b in zip(Ws[:-1], bs[:-1]):
        h = torch.nn.functional.elu(torch.nn.functional.linear(h, W, b))
    sp = (x * torch.nn.functional.linear(h, Ws[-1], bs[-1])).sum(1, keepdim=True)
    q = None
    cot = (e * sp).sum()
    if mode != "value":
        q, = torch.autograd.grad(sp.sum(), x, create_graph=True)
        if r is not None:
            cot = cot + (r * q).sum()
    grads = torch.autograd.grad(cot, [tau] + Ws + bs)
    return [None if o is None else o.detach().double().cpu().numpy() for o in (sp, q) + tuple(grads)]


def core_errors(got, want):
    """Per-output rel-L2 against the fp64 outputs; None where the output is not formed or its fp64 value is
    exactly zero (such an output has to come back exactly zero, which the caller asserts)."""
    return [None if w is None or not np.any(w) else rel_l2(g, w) for g, w in zip(got, want)]


class _NumpyCore(torch.autograd.Function):
    """The restated core inside torch's graph (CPU, fp64): what fit._PISCore is on the device."""

    @staticmethod
    def forward(ctx, grad, mutant, tau, x, *params):
        ps = [p.detach().numpy() for p in params]
        ctx.Ws, ctx.mutant, ctx.grad = ps[0::2], mutant, grad
        sp, q, ctx.st = core_forward(ps[0::2], ps[1::2], tau.detach().numpy(), x.detach().numpy(), grad, mutant)
        q = torch.from_numpy(np.ascontiguousarray(q)) if grad else x.new_empty(0, x.shape[1])
        if not grad:
            ctx.mark_non_differentiable(q)
        return torch.from_numpy(sp), q

    @staticmethod
    def backward(ctx, g_sp, g_q):
        r = g_q.numpy() if ctx.grad and g_q is not None else None
        dWs, dbs, taubar = core_backward(ctx.Ws, ctx.st, g_sp.numpy(), r, ctx.mutant)
        grads = [torch.from_numpy(np.ascontiguousarray(g)) for pair in zip(dWs, dbs) for g in pair]
        return (None, None, torch.from_numpy(np.ascontiguousarray(taubar)), None) + tuple(grads)


def restated_objective(beta, loss_fn, c, nx, mutant=None):
    """The objective around the core (the issue's split): t_encoder, smooth_net and the embedding in torch
    with ordinary autograd, the g0 part under no_grad from the equation's closed forms, the loss of
    fit.gradient_objective with FixedLossScaler(c) (c <= 1e-9: fit.value_objective)."""
    grad = c > 1e-9

    def objective(net, tx, y):
        eq = net.g0.__self__
        t, x = tx[:, :1], tx[:, 1:]
        lbd = net.T - t
        s = net.smoothing_function(lbd)
        tau = net.t_encoder(net.get_pis_timestep_embedding(lbd))
        with torch.no_grad():
            cf = torch.exp(-0.5 * lbd)
            res, res_x = eq.g(cf * x), cf * eq.g_x(cf * x)
        params = [p for m in net.nn_module if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
        sp, q = _NumpyCore.apply(grad, mutant, tau, x, *params)
        w = torch.exp(beta * t)
        v_loss = torch.mean(w * loss_fn(s * sp + (1.0 - s) * res - y[:, :1]), dim=0)
        if not grad:
            return v_loss, {}
        g_loss = torch.mean(w * loss_fn(s * q + (1.0 - s) * res_x - y[:, 1:1 + nx]), dim=0)
        return v_loss + c * g_loss.sum(dim=-1, keepdim=True), {"train_value_loss": v_loss}
    return objective


def make_equation(case):
    """OUProcessEquation with a seeded two-component mixture (g = -log p, g_x closed forms)."""
    nx, T = case[1], case[3]
    g = torch.Generator().manual_seed(3000 + nx)
    return OUProcessEquation(nx=nx, T=T, num_components=2, mean=torch.randn(2, nx, generator=g, dtype=torch.float64),
                             var=2.0 * torch.ones(2, nx, dtype=torch.float64),
                             pi=torch.tensor([0.4, 0.6], dtype=torch.float64))


def make_net(case, dtype=torch.float64, device="cpu"):
    """PISGradNet of the case: torch's default init plus a seeded N(0, 1) perturbation, of 0.3 on every
    bias and on the phase and of 1 / sqrt(fan_in) on every weight (the size of the default init, so the
    activations of the 512-wide nets stay O(1)); made in fp32, then cast."""
    k = CASES.index(case)
    torch.manual_seed(1000 + k)
    net = PISGradNet(list(case[2]), case[1], make_equation(case).g, T=case[3])
    g = torch.Generator().manual_seed(4000 + k)
    with torch.no_grad():
        for p in net.parameters():
            scale = 0.3 if p.ndim == 1 or p.shape[0] == 1 else p.shape[1] ** -0.5
            p.add_(scale * torch.randn(p.shape, generator=g))
    return net.to(dtype=dtype, device=device)


def param_names(case):
    return [n for n, _ in make_net(case).named_parameters()]


@functools.lru_cache(maxsize=None)
def make_batch(k):
    """(tx, y (B, 1 + nx), clip or None) of case k as fp32 tensors on the CPU: t uniform on [0, T), x seeded
    normals, and the labels the fp64 network's own (u, grad_x u) plus NOISE x their rms x N(0, 1), value
    and gradient columns apart.  u is ~ nx through g0 = -log p: labels of size 1 would make the value
    residual u itself and bury the gradient losses the gates look at, while residuals far below u make
    u - y cancel in fp32 (NOISE 0.1: torch's own fp32 gradients are up to 1e-4 from fp64 on the CPU, the
    parity bar itself; 0.3: 3.2e-5 at most).  The clip is the median |residual| of the fp64 run, so both
    branches of rho are taken."""
    case = CASES[k]
    B, nx, widths, T, beta, clipped, c = case
    g = torch.Generator().manual_seed(2000 + k)
    tx = torch.cat([torch.rand(B, 1, generator=g) * T, torch.randn(B, nx, generator=g)], 1)
    u, u_tx = fit._u_and_grad(make_net(case), tx.double())
    out = torch.cat([u.detach(), u_tx.detach()[:, 1:]], 1)
    rms = lambda a: a.square().mean().sqrt()  # noqa: E731
    scale = torch.cat([rms(out[:, :1]).reshape(1), rms(out[:, 1:]).expand(nx)])
    y = (out + NOISE * scale * torch.randn(B, 1 + nx, generator=g)).float()
    clip = None
    if clipped:
        res = [u.detach() - y[:, :1].double()]
        if c > 1e-9:
            res.append(u_tx.detach()[:, 1:] - y[:, 1:1 + nx].double())
        clip = float(np.float32(torch.cat(res, 1).abs().median()))
    return tx, y, clip


def loss_fn_of(clip):
    return torch.square if clip is None else fit.LossFnLinearClip(clip)


def torch_objective(case, clip):
    """The existing torch objective of the case: what TRAIN.BACKEND: torch runs."""
    beta, c, nx = case[4], case[6], case[1]
    if c <= 1e-9:
        return fit.value_objective(beta, loss_fn_of(clip))
    return fit.gradient_objective(beta, loss_fn_of(clip), fit.FixedLossScaler(c), nx)


def run(objective, net, k, dtype, device):
    """(loss, gradients of net.parameters() in order) of `objective` on case k's batch, as fp64 numpy."""
    tx, y, _ = make_batch(k)
    loss, _ = objective(net, tx.to(dtype=dtype, device=device), y.to(dtype=dtype, device=device))
    assert loss.shape == (1,)
    loss.sum().backward()
    return float(loss.detach().double().sum()), [p.grad.detach().double().cpu().numpy() for p in net.parameters()]


def torch_result(k, dtype, device):
    case = CASES[k]
    return run(torch_objective(case, make_batch(k)[2]), make_net(case, dtype, device), k, dtype, device)


@functools.lru_cache(maxsize=None)
def torch_fp64(k):
    """The yardstick: torch fp64 autograd of the whole PISGradNet on the CPU, computed once per case."""
    return torch_result(k, torch.float64, "cpu")


def restated(k, mutant=None, zero_unit=False):
    """The restatement on case k.  zero_unit: the last unit of nn_module's last hidden layer has zero
    weights and bias (a structural error the gates must see)."""
    case = CASES[k]
    net = make_net(case)
    if zero_unit:
        lin = [m for m in net.nn_module if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            lin[-2].weight[-1].zero_()
            lin[-2].bias[-1].zero_()
    return run(restated_objective(case[4], loss_fn_of(make_batch(k)[2]), case[6], case[1], mutant), net, k,
               torch.float64, "cpu")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def tensor_errors(got, want):
    """Per-tensor rel-L2 of `got` against `want`; a tensor whose wanted gradient is exactly zero
    (smooth_net's last bias: out(lambda) - out(0) cancels it) is measured against the largest gradient
    norm of the case instead of its own."""
    top = max(float(np.linalg.norm(w)) for w in want)
    out = []
    for g, w in zip(got, want):
        nw = float(np.linalg.norm(w))
        out.append(float(np.linalg.norm(np.asarray(g, np.float64) - w)) / (nw if nw > 0.0 else top))
    return out


def worst_rel_l2(got, want):
    return max(tensor_errors(got, want))
