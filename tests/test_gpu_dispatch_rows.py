"""Every row of the path-kernel unit table (csrc/dpi_route.h DPI_UNITS), one tiny labelling call
per kernel instance the row can launch, against the fp64 oracle (oracle/dpi_oracle.py).

Rows: {Cha, OU, GBM} x {ELU, Tanh} x {plain, TD, wide} and the two fused-baseline rows (Cha / OU
through sample_with_gradients).  Nets per row: widths [16] (only the fp32 instance exists), [32, 32]
in the exact-fp32 and the default fp16-split mode (both instances), and ZeroSolution on the ELU rows
(the Tanh units hold no zero-net instance).  On the fused-baseline rows [32, 32] in the default mode
and ZeroSolution take the one-launch form; the other two nets run the two launches it replaces.

Shapes: n = 3 points, M = 128 paths (two 64-path blocks per point, so the cross-block reduce runs),
K = 2 Euler steps; nx = 7 on the narrow rows (no multiple of 4 or 16: the padding lanes are live)
and 129 on the wide ones (the first width past NXP_MAX = 128); TD rows at estimate_delta_t = 0.3,
where the three uniform times fall on both sides of t + dt < T; GBM with the full Hessian diagonal
(no SDGD).  Tolerance: the suite's rel-L2 < 1e-4 on the value column and on the gradient block.

These nets stand at torch's default initialisation, where the network adds 1e-5 .. 1e-2 of the label:
tests/test_gpu_network_phase.py runs the same rows with nets whose share of the label is gated on the
CPU, and is the test that is sensitive to the network phase."""
import numpy as np
import pytest
import torch

import deeppicarditeration_amd as dpi
from deeppicarditeration_amd import _lib as L
from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
N, M, K, SEED, EPOCH, DT = 3, 128, 2, 1, 1, 0.3

ROWS = [(eq, act, var) for var in ("plain", "td", "wide") for act in ("ELU", "Tanh") for eq in ("cha", "ou", "gbm")]
ROWS += [("cha", "ELU", "fb"), ("ou", "ELU", "fb")]
NETS = ["w16", "w32x2-f32", "w32x2-auto", "zero"]
CASES = [(*row, net) for row in ROWS for net in NETS if net != "zero" or row[1] == "ELU"]


def test_the_rows_are_the_unit_table():
    assert len(ROWS) == len(set(ROWS)) == 20


def _equation(kind, nx):
    rng = np.random.default_rng(nx)
    if kind == "cha":
        return dpi.Cha(nx, 1.0, 5.0, 1.0), O.Cha(nx, 1.0, 5.0, 1.0)
    if kind == "ou":
        C = 3
        mean, var, pi = rng.uniform(-1, 1, (C, nx)), np.full((C, nx), 2.0), rng.uniform(0.1, 1, C)
        pi = pi / pi.sum()
        eq = dpi.OUProcessEquation(nx=nx, T=1.0, alpha=1.0, num_components=C, mean=mean, var=var, pi=pi, alpha_scale=4.0)
        return eq, O.OUProcessEquation(nx, mean, var, pi, alpha_scale=4.0)
    w = rng.standard_normal((2, 1 + nx)) / np.sqrt(nx)
    w[:, 0] = 1.0
    eq = dpi.GBMEquationComplexExact(nx, 1.0, 1.0, w=w, v=rng.standard_normal((2, 1)))
    return eq, O.GBMEquationComplexExact(nx, eq.w.numpy(), eq.v.numpy())


def _net(eq, net, act):
    if net == "zero":
        return dpi.ZeroSolution(1), O.ZeroNet()
    widths = [16] if net == "w16" else [32, 32]
    torch.manual_seed(17)
    m = dpi.construct_mlp(1 + eq.nx, 1, widths, [act] * len(widths), None)
    lin = [l for l in m if isinstance(l, torch.nn.Linear)]
    return m, O.MLP([l.weight.detach().double().numpy() for l in lin], [l.bias.detach().double().numpy() for l in lin],
                    [act] * len(widths))


@pytest.mark.parametrize("eq_kind,act,variant,net", CASES, ids=["-".join(c) for c in CASES])
def test_unit_row_vs_oracle(eq_kind, act, variant, net):
    nx = 129 if variant == "wide" else 7
    dt = DT if variant == "td" else 0.0
    eq, oeq = _equation(eq_kind, nx)
    module, onet = _net(eq, net, act)
    lib = L.load()
    L.check(lib.dpi_set_gemm_precision(L.DPI_GEMM_F32 if net.endswith("f32") else L.DPI_GEMM_AUTO), "gemm precision")
    try:
        gen = dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=M,
                                      n_estimate_integral=M, n_euler_steps=K, seed=SEED, epoch=EPOCH,
                                      estimate_delta_t=dt if dt else None)
        if variant == "fb":  # points and labels in one call: one launch where the fused baseline fits
            tx, y = gen.sample_with_gradients(N)
            otx, ref = O.sample_with_gradients(oeq, onet, N, M, K, SEED, EPOCH, 0)
            assert np.allclose(tx.cpu().numpy(), otx, rtol=0, atol=2e-5)
        else:  # baseline launch, then the row's path launch
            tx, pb = gen.sample_t_and_x(N, point_base=0)
            y = gen.generate_with_gradients(tx, point_base=pb)
            if dt:
                t = tx[:, 0].cpu().numpy()
                assert (t + dt < 1).any() and (t + dt >= 1).any()  # t = 0.81, 0.06, 0.18
            ref = O.labels_grad(oeq, onet, tx.cpu().double().numpy(), M, K, SEED, EPOCH, 0, delta_t=dt)
        y = y.cpu().numpy()
    finally:
        L.check(lib.dpi_set_gemm_precision(L.DPI_GEMM_AUTO), "gemm precision")
    parts = O.rel_l2_parts(y, ref)
    print(eq_kind, act, variant, net, parts)
    assert np.isfinite(y).all()
    assert parts["value"] < TOL and parts["grad"] < TOL, parts
