"""The general MLP family of the path kernel (csrc/dpi_general.h): first-order Cha /
OU labels of any construct_mlp value network of 1..8 hidden layers, each 1..256 wide, all-ELU or
all-Tanh, that has no specialised kernel instance — against the fp64 oracle (oracle/dpi_oracle.py).

Shapes as tests/test_gpu_dispatch_rows.py: n = 3 points, M = 128 paths (two 64-path blocks per point,
so the cross-block reduce runs), K = 2 Euler steps, nx = 7 (the padding lanes are live), seed 1,
epoch 1.  Tolerance: the suite's rel-L2 < 1e-4 on the value column and on the gradient block; all
labels finite.

Nets: torch.manual_seed(17), construct_mlp, then the hidden-to-hidden weights x 2 and the output
weight and bias x 8: at torch's default initialisation a deep net adds only 1e-4..1e-3 of the label,
and a wrong network phase could pass.  Every oracle case first asserts on the CPU that the net matters:
the oracle's labels with ZeroNet differ from those with the net by rel-L2 >= 1e-2 on the gradient
block and >= 1e-3 on the value column."""
import ctypes

import numpy as np
import pytest
import torch

import deeppicarditeration_amd as dpi
from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd._lib import DPIError
from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
N, M, K, SEED, EPOCH = 3, 128, 2, 1, 1

WIDTHS = [[40], [20, 20, 20], [64] * 4, [128] * 5, [100, 50, 20, 50, 100, 30, 10, 5], [256] * 2, [129, 200, 256],
          [256] * 8]
CASES = [(eq, act, tuple(w), 7) for eq in ("cha", "ou") for act in ("ELU", "Tanh") for w in WIDTHS]
CASES += [(eq, act, tuple(w), nx) for eq in ("cha", "ou") for act in ("ELU", "Tanh") for w in ([64] * 4, [256] * 8)
          for nx in (100, 128)]


def _wid(w):
    return "x".join(map(str, w)) if len(set(w)) > 1 else f"{len(w)}x{w[0]}"


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
    return dpi.GBMEquationComplexExact(nx, 1.0, 1.0, w=w, v=rng.standard_normal((2, 1))), None


def _net(nx, widths, act):
    """The module (weights scaled so that the net matters) and its oracle twin."""
    torch.manual_seed(17)
    m = dpi.construct_mlp(1 + nx, 1, list(widths), [act] * len(widths), None)
    lin = [l for l in m if isinstance(l, torch.nn.Linear)]
    with torch.no_grad():
        for l in lin[1:-1]:
            l.weight.mul_(2.0)
        lin[-1].weight.mul_(8.0)
        lin[-1].bias.mul_(8.0)
    onet = O.MLP([l.weight.detach().double().numpy() for l in lin], [l.bias.detach().double().numpy() for l in lin],
                 [act] * len(widths))
    return m, onet


def _gen(eq, module, M_=M, K_=K, **kw):
    return dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=M_,
                                   n_estimate_integral=M_, n_euler_steps=K_, seed=SEED, epoch=EPOCH, **kw)


def _family(gen, td=False):
    return gen.net.family(gen.problem, td)


def _net_matters(oeq, onet, txh, M_, K_, pb=0):
    ref = O.labels_grad(oeq, onet, txh, M_, K_, SEED, EPOCH, pb)
    zero = O.labels_grad(oeq, O.ZeroNet(), txh, M_, K_, SEED, EPOCH, pb)
    d = O.rel_l2_parts(zero, ref)
    assert d["grad"] >= 1e-2 and d["value"] >= 1e-3, ("the net does not matter to these labels", d)
    return ref


def _check(y, ref, what):
    parts = O.rel_l2_parts(y, ref)
    print(what, parts)
    assert np.isfinite(y).all()
    assert parts["value"] < TOL and parts["grad"] < TOL, parts


@pytest.mark.parametrize("eq_kind,act,widths,nx", CASES, ids=[f"{e}-{a}-{_wid(w)}-nx{nx}" for e, a, w, nx in CASES])
def test_general_net_vs_oracle(eq_kind, act, widths, nx):
    eq, oeq = _equation(eq_kind, nx)
    module, onet = _net(nx, widths, act)
    gen = _gen(eq, module)
    assert _family(gen) == L.DPI_FAMILY_GENERAL and gen.net.desc.endswith("-general")
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ref = _net_matters(oeq, onet, tx.cpu().double().numpy(), M, K)
    y = gen.generate_with_gradients(tx, point_base=pb).cpu().numpy()
    _check(y, ref, (eq_kind, act, widths, nx))


def test_partial_block():
    """M = 100: the second block of every point has 36 live lanes."""
    eq, oeq = _equation("cha", 7)
    module, onet = _net(7, [128] * 5, "ELU")
    gen = _gen(eq, module, M_=100, partial_blocks=True)
    assert _family(gen) == L.DPI_FAMILY_GENERAL
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ref = _net_matters(oeq, onet, tx.cpu().double().numpy(), 100, K)
    _check(gen.generate_with_gradients(tx, point_base=pb).cpu().numpy(), ref, "partial block")


def test_shard_invariance():
    """label_moments over [0, 64) and [64, 128) + moments_reduce == the single call, bit for bit."""
    eq, _ = _equation("ou", 7)
    module, _ = _net(7, [256] * 2, "Tanh")
    gen = _gen(eq, module)
    assert _family(gen) == L.DPI_FAMILY_GENERAL
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ws = gen.point_baseline(tx)
    full = gen.label_moments(tx, pb, M, 0, M, L.DPI_BOTH, ws)
    parts = torch.stack([gen.label_moments(tx, pb, M, 0, 64, L.DPI_BOTH, ws),
                         gen.label_moments(tx, pb, M, 64, M, L.DPI_BOTH, ws)]).contiguous()
    red = gen.moments_reduce(parts)
    assert torch.isfinite(full).all() and torch.equal(red, full)


def test_stash_reuse():
    """4 points x 1,024 blocks = 4,096 blocks on a fixed number of stash slots (several launches of
    block ranges), more than 64 blocks per point (the k_reduce launch, not the fused reduce): point 0
    against the oracle, and the whole call bit-identical to four one-point calls."""
    n, M_ = 4, 65536
    eq, oeq = _equation("cha", 7)
    module, onet = _net(7, [24] * 5, "ELU")
    gen = _gen(eq, module, M_=M_, K_=1)
    assert _family(gen) == L.DPI_FAMILY_GENERAL
    slots = gen.net.general_slots()
    assert slots > 0 and n * (M_ // 64) > 2 * slots
    tx, pb = gen.sample_t_and_x(n, point_base=0)
    y = gen.generate_with_gradients(tx, point_base=pb)
    ref = _net_matters(oeq, onet, tx[:1].cpu().double().numpy(), M_, 1)
    _check(y[:1].cpu().numpy(), ref, "stash reuse, point 0")
    for i in range(n):
        yi = gen.generate_with_gradients(tx[i:i + 1].contiguous(), point_base=pb + i)
        assert torch.equal(yi, y[i:i + 1]), i


def test_canary():
    """8 x 256, M = 100 (a partial block): nothing is written past the workspace (whose last region is
    the stash), the moments or the labels (the pattern of tests/test_gpu_canary.py)."""
    from test_gpu_canary import Carved, _stream
    nx, n, M_ = 7, 3, 100
    eq, _ = _equation("ou", nx)
    module, _ = _net(nx, [256] * 8, "ELU")
    gen = _gen(eq, module, M_=M_, partial_blocks=True)
    F = 1 + nx
    c = Carved(ws=gen.workspace_bytes(n, M_), mom=n * 2 * F * 4, y=n * F * 4)
    tx, pb = gen.sample_t_and_x(n, point_base=11)
    gen.point_baseline(tx, ws=c.u8("ws"))
    args = (gen.problem, gen.net.handle, ctypes.c_void_p(tx.data_ptr()), n, M_, gen.K, gen.seed, gen.epoch, pb)
    L.check(gen.lib.dpi_label_moments_finalize(*args, L.DPI_BOTH, float("inf"), c.ptr("y"), c.ptr("mom"), c.ptr("ws"),
                                               c.nbytes("ws"), _stream()), "moments_finalize")
    c.check()
    assert torch.isfinite(c.f32("mom", n, 2, F)).all() and torch.isfinite(c.f32("y", n, F)).all()


def test_workspace_does_not_grow_with_the_stash():
    """workspace_bytes(n, 64 k) is affine in k with the slope of a 4 x 128 net at the same nx: the
    stash is a constant."""
    eq, _ = _equation("cha", 100)
    g_gen = _gen(eq, _net(100, [256] * 8, "ELU")[0])
    g_spec = _gen(eq, _net(100, [128] * 4, "ELU")[0])
    n = 16
    a = [g_gen.workspace_bytes(n, 64 * k) for k in (1, 2, 5, 64, 1024)]
    b = [g_spec.workspace_bytes(n, 64 * k) for k in (1, 2, 5, 64, 1024)]
    assert [x - a[0] for x in a] == [x - b[0] for x in b]
    assert a[0] > b[0]


@pytest.mark.parametrize("what", ["gbm", "td", "nx129"])
def test_refusals_name_their_cap(what):
    nx = 129 if what == "nx129" else 7
    eq, _ = _equation("gbm" if what == "gbm" else "cha", nx)
    module, _ = _net(nx, [128] * 5, "ELU")
    gen = _gen(eq, module, estimate_delta_t=0.3 if what == "td" else None)
    word = {"gbm": "GBM", "td": "TD", "nx129": "128"}[what]
    with pytest.raises(DPIError, match=word) as ei:
        gen.generate_with_gradients(*gen.sample_t_and_x(N, point_base=0))
    assert f"({L.DPI_ERR_UNSUPPORTED})" in str(ei.value)
    with pytest.raises(DPIError, match=word):
        _family(gen, td=what == "td")


@pytest.mark.parametrize("widths,word", [([16] * 9, "8"), ([16, 257], "256")])
def test_upload_refusals(widths, word):
    lib = L.load()
    w = (ctypes.c_int * len(widths))(*widths)
    rc = lib.dpi_net_create_mlp(8, len(widths), w, L.DPI_ACT_ELU, (ctypes.c_float * 1)(), 1,
                                ctypes.byref(ctypes.c_void_p()))
    assert rc == L.DPI_ERR_UNSUPPORTED and word in L.last_error()


TRAIN = """NAME: {name}
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
  N_EPOCHS: 4
  BATCH_SIZE: 128
  SUPERVISE_GRADIENT: true
  LOSS: {{beta: 0.0, SCALER: {{cls: FixedLossScaler, kwargs: {{fixed_weight: 0.1}}}}}}
  OPTIMIZER: {{kwargs: {{lr: 0.003}}}}
NETWORK:
  NEURONS: [24, 24, 24, 24, 24]
  ACTIVATIONS: [Tanh, Tanh, Tanh, Tanh, Tanh]
  BOUND: None
  RELOAD: true
EVAL: {{L2_N_POINTS: 256}}
"""


def test_picard_train_with_a_five_layer_net(tmp_path):
    """`picard train` with NETWORK.NEURONS [24] * 5: iteration 2's labels come from the trained
    five-layer iterate through the general family."""
    from deeppicarditeration_amd.config import load_cfg
    from deeppicarditeration_amd.runner import PicardRunner
    f = tmp_path / "cha5.yaml"
    f.write_text(TRAIN.format(name=tmp_path / "run"))
    runner = PicardRunner(load_cfg(str(f)))
    seen = {}
    orig = runner.labels

    def labels():
        tx, y = orig()
        seen[runner.i] = (type(runner.u_current).__name__, y.detach().clone())
        return tx, y

    runner.labels = labels
    hist = runner.run()
    assert [h["iter"] for h in hist] == [1, 2] and all(h["labels"] == 512 for h in hist)
    assert seen[2][0] == "Sequential"
    assert all(torch.isfinite(y).all() for _, y in seen.values())
    assert all(h["rel_l2_u"] is not None and h["rel_l2_u"] == h["rel_l2_u"] for h in hist)
