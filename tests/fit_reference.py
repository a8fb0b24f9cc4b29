"""The fit's loss and parameter gradients restated in numpy fp64 (forward, adjoint,
loss seeds, tangent of the adjoint chain, reverse), the case table the CPU and GPU tests of the device
fit share, and the torch side of the comparison (fit.gradient_objective / fit.value_objective under
autograd).  No GPU and no library is needed to import this module."""
import functools

import numpy as np
import torch

from deeppicarditeration_amd import fit
from deeppicarditeration_amd.solution import construct_mlp

# (B, nx, hidden widths, activation, beta, clip?, c, y row stride beyond 1 + nx)
# B: 1, a whole tile, one row past it, a partial second tile, 8 tiles.  Nets: one layer, the r03c [32, 32],
# the shipped 4 x 128, the deepest narrow one, widths that are no multiple of the unit block or the weight
# tile (65, 129), and the largest (8 x 256 at nx = 256) once.  c = 0 is the value kind.
CASES = [
    (1, 7, [16], "ELU", 0.0, False, 1.0, 0),
    (64, 7, [32, 32], "Tanh", 0.7, False, 1.0, 0),
    (65, 7, [32, 32], "ELU", 0.7, True, 0.1, 0),
    (100, 7, [65, 65], "Tanh", 0.0, True, 1.0, 0),
    (512, 7, [24] * 8, "ELU", 0.7, False, 1.0, 0),
    (100, 100, [128] * 4, "ELU", 0.0, False, 1.0, 0),
    (512, 100, [128] * 4, "ELU", 0.7, False, 1.0, 0),
    (65, 100, [129], "Tanh", 0.7, True, 0.1, 0),
    (64, 128, [32, 32], "Tanh", 0.0, False, 0.1, 0),
    (100, 128, [65, 65], "ELU", 0.7, True, 1.0, 0),
    (64, 256, [256] * 8, "ELU", 0.0, False, 1.0, 0),
    (1, 100, [128] * 4, "Tanh", 0.7, False, 1.0, 0),
    (65, 7, [16], "Tanh", 0.0, False, 0.0, 0),
    (100, 100, [32, 32], "ELU", 0.7, True, 0.0, 0),
    (512, 128, [129], "ELU", 0.0, False, 0.0, 0),
    (100, 7, [32, 32], "ELU", 0.0, False, 1.0, 49),
    (1, 7, [24] * 8, "Tanh", 0.7, True, 0.1, 0),
    (64, 100, [65, 65], "Tanh", 0.7, False, 1.0, 0),
    (65, 128, [128] * 4, "Tanh", 0.0, True, 1.0, 0),
    (512, 7, [16], "ELU", 0.0, True, 0.1, 0),
    (100, 100, [24] * 8, "ELU", 0.7, False, 0.1, 0),
    (64, 7, [129], "ELU", 0.7, False, 1.0, 0),
    (65, 100, [16], "ELU", 0.0, False, 1.0, 0),
    (512, 100, [65, 65], "ELU", 0.0, True, 1.0, 0),
    (1, 128, [129], "Tanh", 0.0, False, 0.1, 0),
    (100, 7, [128] * 4, "Tanh", 0.7, False, 0.0, 0),
    (64, 100, [32, 32], "ELU", 0.7, True, 1.0, 0),
    (65, 7, [24] * 8, "Tanh", 0.0, False, 1.0, 0),
    (512, 128, [32, 32], "Tanh", 0.7, False, 1.0, 0),
    (100, 128, [16], "ELU", 0.7, True, 0.1, 0),
]
IDS = [f"{k}-B{c[0]}-nx{c[1]}-{len(c[2])}x{max(c[2])}-{c[3]}-b{c[4]}-{'clip' if c[5] else 'sq'}-c{c[6]}"
       + ("-wide_y" if c[7] else "") for k, c in enumerate(CASES)]
GAIN = 2.0  # the hidden weights are torch's default init times this: keeps grad_x u of the deep nets alive


def _phi(act, z):
    """phi, phi', phi'' of ELU (alpha = 1) or Tanh."""
    if act == "ELU":
        e = np.exp(np.minimum(z, 0.0))
        return np.where(z > 0, z, e - 1.0), np.where(z > 0, 1.0, e), np.where(z > 0, 0.0, e)
    a = np.tanh(z)
    return a, 1.0 - a * a, -2.0 * a * (1.0 - a * a)


def _rho(x, clip):
    if clip is None:
        return x * x, 2.0 * x
    inside = np.abs(x) < clip
    return (np.where(inside, x * x, 2.0 * clip * np.abs(x) - clip ** 2),
            np.where(inside, 2.0 * x, 2.0 * clip * np.sign(x)))


def reference(Ws, bs, act, tx, y, beta, clip, c, drop_tangent=False):
    """losses (2 + nx: total, v_loss, g_loss[nx]) and the gradients (dWs, dbs) in the arithmetic of the
    five passes, fp64.  c <= 1e-9 is the value kind (passes 2 and 4 skipped, g_loss = 0).
    drop_tangent: leave pass 4 out (the structural error the gates must see)."""
    Ws = [np.asarray(W, np.float64) for W in Ws]
    bs = [np.asarray(b, np.float64) for b in bs]
    tx, y = np.asarray(tx, np.float64), np.asarray(y, np.float64)
    B, n0 = tx.shape
    nx, L = n0 - 1, len(Ws) - 1
    grad = c > 1e-9
    # 1. forward
    a, d1, d2 = [tx], [None], [None]
    for l in range(L):
        f, g, h = _phi(act, a[-1] @ Ws[l].T + bs[l])
        a.append(f), d1.append(g), d2.append(h)
    u = a[L] @ Ws[L].T + bs[L]  # (B, 1)
    # 3. loss and seeds
    w = np.exp(beta * tx[:, :1])
    r0, dr0 = _rho(u - y[:, :1], clip)
    losses = np.zeros(2 + nx)
    losses[1] = np.mean(w * r0)
    e = w * dr0 / B  # (B, 1)
    dWs = [np.zeros_like(W) for W in Ws]
    zeta = [None] * (L + 1)
    delta = lam = None
    if grad:
        # 2. adjoint, downward
        lam, delta = [None] * (L + 1), [None] * (L + 1)
        lam[L] = np.broadcast_to(Ws[L], (B, Ws[L].shape[1]))
        for l in range(L, 0, -1):
            delta[l] = lam[l] * d1[l]
            lam[l - 1] = delta[l] @ Ws[l - 1]
        rg, drg = _rho(lam[0][:, 1:] - y[:, 1:1 + nx], clip)
        losses[2:] = np.mean(w * rg, axis=0)
        lb = np.concatenate([np.zeros((B, 1)), c * w * drg / B], axis=1)
        # 4. tangent of the adjoint chain, upward
        if not drop_tangent:
            for l in range(1, L + 1):
                db_ = lb @ Ws[l - 1].T
                dWs[l - 1] += delta[l].T @ lb
                lb = db_ * d1[l]
                zeta[l] = db_ * lam[l] * d2[l]
            dWs[L] += lb.sum(axis=0, keepdims=True)
    losses[0] = losses[1] + (c * losses[2:].sum() if grad else 0.0)
    # 5. reverse, downward
    dbs = [None] * (L + 1)
    dWs[L] += e.T @ a[L]
    dbs[L] = e.sum(axis=0)
    abar = e @ Ws[L]
    for l in range(L, 0, -1):
        zb = abar * d1[l] + (zeta[l] if zeta[l] is not None else 0.0)
        dWs[l - 1] += zb.T @ a[l - 1]
        dbs[l - 1] = zb.sum(axis=0)
        abar = zb @ Ws[l - 1]
    return losses, dWs, dbs


def make_net(case, dtype=torch.float64, device="cpu", seed=None):
    """construct_mlp of the case with its seeded fp32 weights (hidden layers scaled by GAIN), cast."""
    B, nx, widths, act = case[:4]
    torch.manual_seed(1000 + (CASES.index(case) if seed is None else seed))
    net = construct_mlp(1 + nx, 1, list(widths), [act] * len(widths), None)
    with torch.no_grad():
        for m in list(net)[:-1]:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(GAIN)
    return net.to(dtype=dtype, device=device)


@functools.lru_cache(maxsize=None)
def make_batch(k):
    """(tx, y (B, stride), clip or None) of case k as fp32 tensors on the CPU: seeded, labels of the size
    of the network's own outputs; the clip is the median |residual| of the fp64 run, so both branches
    of rho are taken."""
    case = CASES[k]
    B, nx, widths, act, beta, clipped, c, extra = case
    g = torch.Generator().manual_seed(2000 + k)
    tx = torch.cat([torch.rand(B, 1, generator=g), torch.randn(B, nx, generator=g)], 1)
    y = torch.randn(B, 1 + nx + extra, generator=g) * 0.5
    clip = None
    if clipped:
        net = make_net(case)
        u, u_tx = fit._u_and_grad(net, tx.double())
        res = [u.detach() - y[:, :1].double()]
        if c > 1e-9:
            res.append(u_tx.detach()[:, 1:] - y[:, 1:1 + nx].double())
        clip = float(np.float32(torch.cat(res, 1).abs().median()))
    return tx, y, clip


class _Recording(fit.FixedLossScaler):
    def scale(self, v_loss, g_loss_multi_dim):
        self.g_loss = g_loss_multi_dim.detach()
        return super().scale(v_loss, g_loss_multi_dim)


def torch_objective(case, clip):
    """The existing torch objective of the case (what TRAIN.BACKEND: torch runs) and its scaler."""
    beta, c, nx = case[4], case[6], case[1]
    loss_fn = torch.square if clip is None else fit.LossFnLinearClip(clip)
    if c <= 1e-9:
        return fit.value_objective(beta, loss_fn), None
    scaler = _Recording(c)
    return fit.gradient_objective(beta, loss_fn, scaler, nx), scaler


def torch_result(k, dtype, device):
    """losses (2 + nx) and the parameter gradients (state-dict order) of the torch objective, as fp64
    numpy arrays."""
    case = CASES[k]
    tx, y, clip = make_batch(k)
    net = make_net(case, dtype, device)
    objective, scaler = torch_objective(case, clip)
    loss, info = objective(net, tx.to(dtype=dtype, device=device), y.to(dtype=dtype, device=device))
    loss.sum().backward()
    nx = case[1]
    losses = np.zeros(2 + nx)
    losses[0] = float(loss.detach().sum())
    if scaler is None:
        losses[1] = losses[0]
    else:
        losses[1] = float(info["train_value_loss"].detach().sum())
        losses[2:] = scaler.g_loss.double().cpu().numpy()
    return losses, [p.grad.detach().double().cpu().numpy() for p in net.parameters()]


@functools.lru_cache(maxsize=None)
def torch_fp64(k):
    """The yardstick: torch fp64 autograd on the CPU, computed once per case."""
    return torch_result(k, torch.float64, "cpu")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def worst_rel_l2(got, want):
    """The largest per-tensor rel-L2 over a list of tensors."""
    return max(rel_l2(g, w) for g, w in zip(got, want))
