"""The fp64 oracle twin of a terminal-enforcing solution (NETWORK.cls PicardSolutionEnforceTerminal,
picard/solution_enforce_terminal.py:9-27), the loader of its fixtures (tests/golden/terminal/*.npz, made
by tests/golden/make_golden_terminal.py) and the nets the GPU tests use.

The oracle (oracle/dpi_oracle.py) asks a net for `value_grad(tx) -> (u, du/dtx, hdiag)`.  The twin wraps
the inner construct_mlp net N and answers as the wrapper's forward does:
    Value:         u = g(x) + (T - t) N,  u_x = g_x(x) + (T - t) dN/dx
    OnlyGradient:  u = 0,                 u_x = g_x(x) + (T - t) N        (N has nx outputs)
d/dt is never read (get_f takes u and u_x only), as in tests/heads_util.HeadNet."""
from pathlib import Path

import numpy as np

import heads_util as H
from oracle import dpi_oracle as O

TERMINAL = Path(__file__).resolve().parent / "golden" / "terminal"
TERMINAL_CASES = sorted(p.stem for p in TERMINAL.glob("*.npz"))


def g_x(eq, x):
    """grad g of the oracle's equations (equations.py:307-309 Cha, :595-596 OU)."""
    if isinstance(eq, O.Cha):
        g = eq.g(x)
        return np.ones_like(x) * (eq.k * g * (1 - g))
    if isinstance(eq, O.OUProcessEquation):
        return -eq.grad_log_prob(x)
    raise ValueError(type(eq).__name__)


class TerminalNet:
    """`inner`: O.MLP (kind "Value") or heads_util.HeadNet with nx outputs (kind "OnlyGradient")."""

    def __init__(self, eq, inner, kind):
        assert kind in ("Value", "OnlyGradient"), kind
        self.eq, self.inner, self.kind = eq, inner, kind

    def value_grad(self, tx, need_hdiag=False):
        assert not need_hdiag, "a terminal-enforcing net has no Hessian labels"
        t, x = tx[:, :1], tx[:, 1:]
        tm = self.eq.T - t
        uN, dN, _ = self.inner.value_grad(tx)
        gx = g_x(self.eq, x)
        if self.kind == "Value":
            u, ux = self.eq.g(x) + tm * uN, gx + tm * dN[:, 1:]
        else:
            assert dN.shape[1] == 1 + self.eq.nx and not uN.any()
            u, ux = np.zeros((tx.shape[0], 1)), gx + tm * dN[:, 1:]
        return u, np.concatenate([np.zeros_like(u), ux], axis=1), None


def inner_net(weights, biases, acts, kind):
    return O.MLP(weights, biases, acts) if kind == "Value" else H.HeadNet(weights, biases, acts)


def from_module(eq, module, acts, kind):
    """The twin of a wrapper's inner Sequential `module` on the oracle equation `eq`."""
    import torch
    lin = [l for l in module if isinstance(l, torch.nn.Linear)]
    return TerminalNet(eq, inner_net([l.weight.detach().double().numpy() for l in lin],
                                     [l.bias.detach().double().numpy() for l in lin], acts, kind), kind)


def zero_inner(twin):
    """The same ansatz around an all-zero N (gate (b): what the labels are without the net)."""
    z = inner_net([np.zeros_like(w) for w in twin.inner.W], [np.zeros_like(b) for b in twin.inner.b], twin.inner.acts,
                  twin.kind)
    return TerminalNet(twin.eq, z, twin.kind)


def load(name):
    with np.load(TERMINAL / f"{name}.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def fixture_net(f, eq):
    sd = {k[3:]: f[k] for k in f if k.startswith("sd_")}
    idx = sorted({int(k.split(".")[0]) for k in sd})
    kind = str(f["type"])
    return TerminalNet(eq, inner_net([sd[f"{i}.weight"] for i in idx], [sd[f"{i}.bias"] for i in idx],
                                     [str(a) for a in f["acts"]], kind), kind)


# ---------------------------------------------------------------------------------- the GPU tests' nets
# Shapes of tests/test_gpu_general_mlp.py: n = 3 points, M = 128 paths, K = 2 steps, seed 1, epoch 1.
N, M, K, SEED, EPOCH = 3, 128, 2, 1, 1
WIDTHS = {"w40": [40], "w64x4": [64] * 4, "w128x4": [128] * 4, "mixed8": [100, 50, 20, 50, 100, 30, 10, 5],
          "w256x2": [256] * 2, "w256x8": [256] * 8}
# (equation, type, activation, widths tag, nx)
GPU_CASES = [(eq, kind, act, w, 7) for eq in ("cha", "ou") for kind in ("Value", "OnlyGradient") for act in ("ELU", "Tanh")
             for w in WIDTHS]
GPU_CASES += [(eq, kind, act, w, nx) for eq in ("cha", "ou") for kind in ("Value", "OnlyGradient") for act in ("ELU", "Tanh")
              for w in ("w64x4", "w256x8") for nx in (100, 128)]

# Powers of two by which a net at torch's default initialisation (seed 17) is scaled so that the ansatz
# and the net each decide a measurable share of the label (tests/test_terminal_gates.py, gates (a) and
# (b), which hold for every case of GPU_CASES with these factors):
# (equation, type) -> (factor on every hidden-to-hidden weight, factor on the output weight and bias).
#
# | equation, type    | hidden | output | gate (b) at x1, x1 (value / gradient), worst case |
# |-------------------|--------|--------|---------------------------------------------------|
# | Cha, Value        | 2      | 8      | 3.4e-2 / 8.3e-2                                   |
# | Cha, OnlyGradient | 2      | 8      | 1.5e-2 / 4.1e-3 (short)                           |
# | OU, Value         | 2      | 64     | 1.3e-6 / 2.5e-5 (short; x2, x8: 6.1e-4 / 1.5e-2)  |
# | OU, OnlyGradient  | 2      | 8      | 2.5e-4 / 3.6e-3 (short)                           |
#
# The OU Value form needs most: its value label is dominated by g = -log p_GMM, O(nx).
SCALES = {("cha", "Value"): (2.0, 8.0), ("cha", "OnlyGradient"): (2.0, 8.0),
          ("ou", "Value"): (2.0, 64.0), ("ou", "OnlyGradient"): (2.0, 8.0)}


def equation(kind, nx):
    """(this build's equation, the oracle's) as tests/test_gpu_dispatch_rows.py builds them."""
    import deeppicarditeration_amd as dpi
    rng = np.random.default_rng(nx)
    if kind == "cha":
        return dpi.Cha(nx, 1.0, 5.0, 1.0), O.Cha(nx, 1.0, 5.0, 1.0)
    C = 3
    mean, var, pi = rng.uniform(-1, 1, (C, nx)), np.full((C, nx), 2.0), rng.uniform(0.1, 1, C)
    pi = pi / pi.sum()
    eq = dpi.OUProcessEquation(nx=nx, T=1.0, alpha=1.0, num_components=C, mean=mean, var=var, pi=pi, alpha_scale=4.0)
    return eq, O.OUProcessEquation(nx, mean, var, pi, alpha_scale=4.0)


def oracle_equation(kind, nx):
    return equation(kind, nx)[1]


def scaled_mlp(eq_kind, kind, act, widths, nx, seed=17, scales=None):
    """construct_mlp at torch's default initialisation, scaled by SCALES[(eq_kind, kind)] (or `scales`)."""
    import torch

    from deeppicarditeration_amd.solution import construct_mlp
    torch.manual_seed(seed)
    m = construct_mlp(1 + nx, 1 if kind == "Value" else nx, widths, [act] * len(widths), None)
    hid, out = scales or SCALES[(eq_kind, kind)]
    lin = [l for l in m if isinstance(l, torch.nn.Linear)]
    with torch.no_grad():
        for l in lin[1:-1]:
            l.weight.mul_(hid)
        lin[-1].weight.mul_(out)
        lin[-1].bias.mul_(out)
    return m


def case_id(c):
    eq, kind, act, w, nx = c
    return f"{eq}-{kind}-{act}-{w}-nx{nx}"


def case_nets(eq_kind, kind, act, wtag, nx):
    """(module, acts) of a GPU case: the inner network the wrapper is built around."""
    widths = WIDTHS[wtag]
    return scaled_mlp(eq_kind, kind, act, widths, nx), [act] * len(widths)


def gate_parts(oeq, twin, tx, M_=M, K_=K, pb=0):
    """Oracle labels with the ansatz, and what gates (a) and (b) compare them with: rel-L2 parts of the
    bare inner network's labels (OnlyGradient: the plain head net's) and of the ansatz around an all-zero
    N, both against the ansatz labels."""
    lab = lambda net: O.labels_grad(oeq, net, tx, M_, K_, SEED, EPOCH, pb)  # noqa: E731
    ref = lab(twin)
    return ref, O.rel_l2_parts(lab(twin.inner), ref), O.rel_l2_parts(lab(zero_inner(twin)), ref)


def assert_gates(a, b, what=""):
    assert a["value"] >= 1e-2 and a["grad"] >= 1e-2, ("gate (a): the ansatz does not matter to these labels", what, a)
    assert b["value"] >= 1e-3 and b["grad"] >= 1e-2, ("gate (b): the net does not matter to these labels", what, b)
