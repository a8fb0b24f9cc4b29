"""The phase order of the split first-order path kernels (csrc/dpi_device.h paths_body, DPI_ORDER).

A path block runs integral rollout -> MLP -> terminal rollout ("terminal last") or terminal rollout ->
integral rollout -> MLP with its terminal sums parked in the workspace across the MLP ("terminal first,
parked").  The order decides when a block does its work, never what it computes: same counters, same
per-lane arithmetic, the sums through memory unchanged.  So every policy gives the same bits:

  DPI_ORDER = 4 all terminal-last (the order every split block ran before), 5 all terminal-first parked,
  0 the default (all terminal-first parked), 1 the two workgroups of a CU in opposite orders
  (workgroup-slot parity), 2 block-index parity (both orders inside one point, whatever slots the
  hardware hands out to a grid this small).

Shapes: the smallest at which the park and the orders can go wrong — 3 points; M = 128 (two blocks per
point) and M = 100 (dead lanes in the last block); nx = 100 (the 7/6/6/6 split) and nx = 7 (two
dim-blocks: two waves park and reload nothing); K = 3 and K = 70 (two table chunks).  The workspace checks
need an MLP net handle, which only a device can create, so they are GPU tests too; the zero-net part of
them runs without one."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import deeppicarditeration_amd as dpi
import noise_table_cases as C
from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd import data as D

N, PB, SEED, EPOCH = 3, 5, 11, 2
ORDERS = ("4", "5", "0", "1", "2")  # the first is the reference of the comparison
FLAGS = (L.DPI_BOTH, L.DPI_TERMINAL, L.DPI_INTEGRAL)
# the park of include/dpi.h dpi_workspace_bytes: DPI_PARK_MAX_BLOCKS rows, one per 64-path block of a call
PARK_ROW_BYTES = 4 * 64 * 8 * 4 * 4
PARK_MAX_BLOCKS = L.DPI_PARK_MAX_BLOCKS


def _equation(kind, nx):
    if kind == "cha" or nx == 100:
        return C.equations(kind, nx)[0]
    # the mixture's files ship for nx = 100 only: parameters of the same scale from a fixed seed
    rng = np.random.default_rng(nx)
    pi = rng.uniform(0.5, 1.5, 5)
    return dpi.OUProcessEquation(nx=nx, T=1.0, alpha=1.0, num_components=5, mean_scale=1.0, var_scale=2.0,
                                 alpha_scale=4.0, mean=rng.normal(0.0, 1.0, (5, nx)),
                                 var=rng.uniform(1.0, 3.0, (5, nx)), pi=pi / pi.sum())


def _generator(kind, act, f32, nx, M, K):
    torch.manual_seed(nx + 1000 * K)
    net = dpi.construct_mlp(1 + nx, 1, [128] * 4, [act] * 4, None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", D.PartialBlockNote)
        gen = dpi.OnlineDataGenerator(_equation(kind, nx), net, 1, 1, device="cuda:0", t_always_uniform=True,
                                      n_estimate_terminal=M, n_estimate_integral=M, n_euler_steps=K, seed=SEED,
                                      epoch=EPOCH, partial_blocks=M % 64 != 0)
    if f32:
        gen.use_fp32()
    return gen


def _sample(gen, n, pb, flags):
    """dpi_sample_with_gradients with the estimator flags the generator surface fixes to DPI_BOTH: the
    one-launch k_paths_fb where the pair has one (split ELU nets, not OU 4 x 128), else two launches."""
    F, M = 1 + gen.equation.nx, gen.n_estimate_integral
    ws = gen._workspace(n, M)
    tx, y = (torch.empty(n, F, dtype=torch.float32, device="cuda:0") for _ in range(2))
    mom = torch.empty(n, 2, F, dtype=torch.float32, device="cuda:0")
    gen._configure_problem()
    L.check(gen.lib.dpi_sample_with_gradients(gen.problem, gen.net.handle, n, M, gen.K, gen.seed, gen.epoch, pb,
                                              gen.eps, gen.t_factors, flags, float("inf"), D._ptr(tx), D._ptr(y),
                                              D._ptr(mom), D._ptr(ws), ws.numel(), D._stream(gen._device)),
            "dpi_sample_with_gradients")
    return tx, y, mom


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [100, 7])
@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32"])
@pytest.mark.parametrize("act", ["ELU", "Tanh"])
@pytest.mark.parametrize("kind", ["cha", "ou"])
def test_label_moments_do_not_depend_on_the_phase_order(kind, act, f32, nx, monkeypatch):
    for M in (128, 100):
        for K in (3, 70):
            gen = _generator(kind, act, f32, nx, M, K)
            tx, _ = gen.sample_t_and_x(N, point_base=PB)
            ws = gen.point_baseline(tx)
            for flags in FLAGS:
                want = None
                for order in ORDERS:
                    monkeypatch.setenv("DPI_ORDER", order)
                    got = (gen.label_moments(tx, PB, M, 0, M, flags, ws),) + _sample(gen, N, PB, flags)
                    torch.cuda.synchronize()
                    assert all(torch.isfinite(g).all() for g in got)
                    want = got if want is None else want
                    for g, w in zip(got, want):
                        assert torch.equal(g, w), (M, K, flags, order)
                # both kernels label the same points from the same counters
                assert torch.equal(want[1], tx) and torch.equal(want[0], want[3])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cha", "ou"])
def test_ten_calls_on_one_workspace_reuse_the_park_and_the_tickets(kind, monkeypatch):
    """The park rows and the fused reduce's tickets are reused from call to call, under one policy and
    across policies: every call returns the first call's bits."""
    gen = _generator(kind, "ELU", False, 100, 100, 3)
    tx, _ = gen.sample_t_and_x(N, point_base=PB)
    ws = gen.point_baseline(tx)
    first = None
    for call in range(10):
        monkeypatch.setenv("DPI_ORDER", ("0", "0", "1", "4", "2")[call % 5])
        y, mom = gen.label_moments_finalize(tx, PB, 100, L.DPI_BOTH, ws)
        got = (y, mom) + _sample(gen, N, PB, L.DPI_BOTH)
        first = got if first is None else first
        for g, w in zip(got, first):
            assert torch.equal(g, w), call
    assert torch.equal(first[0], first[3])


@functools.lru_cache(maxsize=None)
def _oracle(case):
    kind, nx, K, M, net = case
    eq, _ = C.equations(kind, nx)
    module, _ = C.nets(net, nx)
    gen = dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=M,
                                  n_estimate_integral=M, n_euler_steps=K, seed=SEED, epoch=EPOCH)
    tx, _ = gen.sample_t_and_x(N, point_base=0)
    _, oeq = C.equations(kind, nx)
    _, onet = C.nets(net, nx)
    ref = C.O.labels_grad(oeq, onet, tx.cpu().numpy().astype(np.float64), M, K, SEED, EPOCH, 0)
    return gen, tx, ref


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["0", "1"])
@pytest.mark.parametrize("case", [("cha", 100, 3, 128, "mlp128x4-split"), ("ou", 100, 3, 128, "mlp64x2-split")],
                         ids=["cha", "ou"])
def test_parked_orders_against_the_fp64_oracle(case, order, monkeypatch):
    """The project's bar for this quantity (tests/test_gpu_parity.py): rel-L2 < 1e-4 on the value column
    and on the gradient block, for k_paths and k_paths_fb."""
    gen, tx, ref = _oracle(case)
    monkeypatch.setenv("DPI_ORDER", order)
    y_paths = gen.generate_with_gradients(tx, point_base=0)
    tx_fb, y_fb = gen.sample_generate(N, 0)
    torch.cuda.synchronize()
    assert torch.equal(tx_fb, tx)
    for y in (y_paths, y_fb):
        parts = C.O.rel_l2_parts(y.cpu().numpy().astype(np.float64), ref)
        print(case, order, parts)
        assert parts["value"] < 1e-4 and parts["grad"] < 1e-4, parts


def _handles(nx=100, widths=None):
    lib = L.load()
    p, net = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.dpi_problem_create_cha(nx, 1.0, 5.0, 1.0, p) == 0
    if widths is None:
        assert lib.dpi_net_create_zero(net) == 0
    else:
        sizes = [1 + nx] + widths + [1]
        n_params = sum(fo * fi + fo for fi, fo in zip(sizes[:-1], sizes[1:]))
        buf = (ctypes.c_float * n_params)()
        assert lib.dpi_net_create_mlp(1 + nx, len(widths), (ctypes.c_int * len(widths))(*widths), L.DPI_ACT_ELU, buf,
                                      n_params, net) == 0, L.last_error()
    return lib, p, net


def test_workspace_without_a_park_is_unchanged():
    """Zero nets park nothing (no MLP phase): the workspace does not step with M inside a 64-path block
    and holds no park row (no device needed)."""
    lib, p, net = _handles()
    try:
        ws = lib.dpi_workspace_bytes
        assert ws(p, net, 16, 100) == ws(p, net, 16, 128) and ws(p, net, 16, 1) == ws(p, net, 16, 64)
        assert ws(p, net, 16, 4096) - ws(p, net, 16, 4032) < PARK_ROW_BYTES
    finally:
        assert lib.dpi_net_destroy(net) == 0 and lib.dpi_problem_destroy(p) == 0


@pytest.mark.gpu
def test_workspace_park_region():
    lib, p, zero = _handles()
    _, p2, mlp = _handles(widths=[128] * 4)
    try:
        ws = lib.dpi_workspace_bytes
        bx = lambda n: (n * 128 * 4 + 255) & ~255  # noqa: E731  (the MLP net's only other region: bx[n][H])
        # unchanged in M within a 64-path block
        assert ws(p2, mlp, 16, 100) == ws(p2, mlp, 16, 128) and ws(p2, mlp, 16, 1) == ws(p2, mlp, 16, 64)
        # a constant: DPI_PARK_MAX_BLOCKS rows whatever n and M, 64 MB at the most
        park = PARK_MAX_BLOCKS * PARK_ROW_BYTES
        assert park <= 64 << 20
        for n, M in ((16, 4096), (32, 4096), (3, 128), (512, 4096)):  # the last: cfg3, above the cap
            assert ws(p2, mlp, n, M) - ws(p, zero, n, M) == bx(n) + park, (n, M)
        # a workspace short by the park is refused before any device work
        need, p16 = ws(p2, mlp, 16, 4096), ctypes.c_void_p(16)

        def moments(ws_bytes):
            return lib.dpi_label_moments(p2, mlp, p16, 16, 4096, 50, 1, 0, 0, 0, 4096, 3, p16, p16, ws_bytes, None)

        assert moments(need - park) == L.DPI_ERR_WORKSPACE
        assert moments(need - 1) == L.DPI_ERR_WORKSPACE
    finally:
        assert lib.dpi_net_destroy(mlp) == 0 and lib.dpi_net_destroy(zero) == 0
        assert lib.dpi_problem_destroy(p) == 0 and lib.dpi_problem_destroy(p2) == 0
