"""Gradient-head networks on the label path (NETWORK.TYPE ValueGradient / OnlyGradient; csrc/dpi_general.h
NetGenHead): first-order Cha / OU labels of a construct_mlp net whose last Linear
outputs grad_x u (1 + nx outputs: u, u_x; nx outputs: u_x, u = 0) against the fp64 oracle given the
same head columns (tests/heads_util.py HeadNet; pinned to the reference by tests/test_heads_oracle.py).

Shapes as tests/test_gpu_general_mlp.py: n = 3 points, M = 128 paths (two 64-path blocks per point, so
the cross-block reduce runs), K = 2 Euler steps, seed 1, epoch 1.  Tolerance: the suite's rel-L2 < 1e-4
on the value column and on the gradient block; all labels finite.

Nets: torch.manual_seed(17), construct_mlp at torch's default initialisation; the eight-layer shapes
(SCALED) get the hidden-to-hidden weights x 2 and the output weights and biases x 8, as _net of
tests/test_gpu_general_mlp.py scales its deep nets.  Every oracle case first asserts on the CPU that
the net matters (measured over these cases: value >= 2.1e-3, gradient >= 4.2e-2):
the oracle's labels with ZeroNet differ from those with the net by rel-L2 >= 1e-2 on the gradient
block and >= 1e-3 on the value column."""
import ctypes
import json

import numpy as np
import pytest
import torch

import deeppicarditeration_amd as dpi
import heads_util as H
from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd._lib import DPIError
from oracle import dpi_oracle as O
from test_gpu_general_mlp import _equation, _wid

pytestmark = pytest.mark.gpu
TOL = 1e-4
N, M, K, SEED, EPOCH = 3, 128, 2, 1, 1
VG, OG = "ValueGradient", "OnlyGradient"

WIDTHS7 = [[40], [128] * 4, [100, 50, 20, 50, 100, 30, 10, 5], [129, 200, 256], [256] * 8]
CASES = [(eq, head, act, tuple(w), 7) for eq in ("cha", "ou") for head in (VG, OG) for act in ("ELU", "Tanh")
         for w in WIDTHS7]
CASES += [(eq, head, "ELU", tuple(w), nx) for eq in ("cha", "ou") for head in (VG, OG) for w in ([64] * 4, [256] * 2)
          for nx in (100, 127, 128)]
SCALED = {(100, 50, 20, 50, 100, 30, 10, 5), (256,) * 8}


def _net(nx, widths, act, head):
    """The module and its oracle twin."""
    torch.manual_seed(17)
    m = dpi.construct_mlp(1 + nx, 1 + nx if head == VG else nx, list(widths), [act] * len(widths), None)
    if tuple(widths) in SCALED:
        lin = [l for l in m if isinstance(l, torch.nn.Linear)]
        with torch.no_grad():
            for l in lin[1:-1]:
                l.weight.mul_(2.0)
            lin[-1].weight.mul_(8.0)
            lin[-1].bias.mul_(8.0)
    return m, H.from_module(m, [act] * len(widths))


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


@pytest.mark.parametrize("eq_kind,head,act,widths,nx", CASES,
                         ids=[f"{e}-{h}-{a}-{_wid(w)}-nx{nx}" for e, h, a, w, nx in CASES])
def test_head_net_vs_oracle(eq_kind, head, act, widths, nx):
    eq, oeq = _equation(eq_kind, nx)
    module, onet = _net(nx, widths, act, head)
    gen = _gen(eq, module)
    assert _family(gen) == L.DPI_FAMILY_GENERAL and gen.net.desc.endswith("-" + head)
    assert gen.net.general_slots() == 0
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ref = _net_matters(oeq, onet, tx.cpu().double().numpy(), M, K)
    y = gen.generate_with_gradients(tx, point_base=pb).cpu().numpy()
    _check(y, ref, (eq_kind, head, act, widths, nx))


@pytest.mark.parametrize("head", [VG, OG])
def test_partial_block(head):
    """M = 100: the second block of every point has 36 live lanes."""
    eq, oeq = _equation("ou", 7)
    module, onet = _net(7, [128] * 4, "ELU", head)
    gen = _gen(eq, module, M_=100, partial_blocks=True)
    assert _family(gen) == L.DPI_FAMILY_GENERAL
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ref = _net_matters(oeq, onet, tx.cpu().double().numpy(), 100, K)
    _check(gen.generate_with_gradients(tx, point_base=pb).cpu().numpy(), ref, "partial block")


@pytest.mark.parametrize("eq_kind,head", [("ou", VG), ("cha", OG)])
def test_shard_invariance(eq_kind, head):
    """label_moments over [0, 64) and [64, 128) + moments_reduce == the single call, bit for bit."""
    eq, _ = _equation(eq_kind, 7)
    module, _ = _net(7, [256] * 2, "Tanh", head)
    gen = _gen(eq, module)
    assert _family(gen) == L.DPI_FAMILY_GENERAL
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ws = gen.point_baseline(tx)
    full = gen.label_moments(tx, pb, M, 0, M, L.DPI_BOTH, ws)
    parts = torch.stack([gen.label_moments(tx, pb, M, 0, 64, L.DPI_BOTH, ws),
                         gen.label_moments(tx, pb, M, 64, M, L.DPI_BOTH, ws)]).contiguous()
    red = gen.moments_reduce(parts)
    assert torch.isfinite(full).all() and torch.equal(red, full)


def test_many_blocks_one_launch():
    """4 points x 1,024 blocks = 4,096 blocks in one path launch (no stash, so no block ranges), more
    than 64 blocks per point (the k_reduce launch, not the fused reduce): point 0 against the oracle,
    and the whole call bit-identical to four one-point calls."""
    n, M_ = 4, 65536
    eq, oeq = _equation("ou", 7)
    module, onet = _net(7, [24] * 3, "ELU", VG)
    gen = _gen(eq, module, M_=M_, K_=1)
    assert _family(gen) == L.DPI_FAMILY_GENERAL and gen.net.general_slots() == 0
    tx, pb = gen.sample_t_and_x(n, point_base=0)
    y = gen.generate_with_gradients(tx, point_base=pb)
    ref = _net_matters(oeq, onet, tx[:1].cpu().double().numpy(), M_, 1)
    _check(y[:1].cpu().numpy(), ref, "many blocks, point 0")
    for i in range(n):
        yi = gen.generate_with_gradients(tx[i:i + 1].contiguous(), point_base=pb + i)
        assert torch.equal(yi, y[i:i + 1]), i


@pytest.mark.parametrize("head", [VG, OG])
def test_workspace_has_no_stash(head):
    """The [256] * 8 Value net carries the general family's stash; the head net of the same widths does
    not, and is smaller by at least that stash (256 slots x 7 layers x 16 tiles x 256 threads x 16 B)."""
    nx, n = 100, 16
    eq, _ = _equation("cha", nx)
    g_head = _gen(eq, _net(nx, [256] * 8, "ELU", head)[0])
    torch.manual_seed(17)
    g_value = _gen(eq, dpi.construct_mlp(1 + nx, 1, [256] * 8, ["ELU"] * 8, None))
    assert _family(g_value) == L.DPI_FAMILY_GENERAL and g_value.net.general_slots() == 256
    a, b = g_head.workspace_bytes(n, M), g_value.workspace_bytes(n, M)
    assert a < b and b - a >= 256 * 7 * 16 * 256 * 16


def test_canary():
    """[256] * 8, ValueGradient, nx = 128 (129 outputs), M = 100 (a partial block): nothing is written
    past the workspace, the moments or the labels (the pattern of tests/test_gpu_canary.py)."""
    from test_gpu_canary import Carved, _stream
    nx, n, M_ = 128, 3, 100
    eq, _ = _equation("ou", nx)
    module, _ = _net(nx, [256] * 8, "ELU", VG)
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


@pytest.mark.parametrize("head", [VG, OG])
@pytest.mark.parametrize("what", ["gbm", "td", "nx129"])
def test_refusals_name_their_cap(what, head):
    nx = 129 if what == "nx129" else 7
    eq, _ = _equation("gbm" if what == "gbm" else "cha", nx)
    module, _ = _net(nx, [40], "ELU", head)
    gen = _gen(eq, module, estimate_delta_t=0.3 if what == "td" else None)
    word = {"gbm": "GBM", "td": "TD", "nx129": "128"}[what]
    with pytest.raises(DPIError, match=word) as ei:
        gen.generate_with_gradients(*gen.sample_t_and_x(N, point_base=0))
    assert f"({L.DPI_ERR_UNSUPPORTED})" in str(ei.value) and "head" in str(ei.value)
    with pytest.raises(DPIError, match=word):
        _family(gen, td=what == "td")


@pytest.mark.parametrize("head", [VG, OG])
def test_hessian_labels_are_refused(head):
    eq, _ = _equation("cha", 7)
    gen = _gen(eq, _net(7, [40], "ELU", head)[0])
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    with pytest.raises(DPIError, match="Hessian") as ei:
        gen.generate_with_gradients_and_hessians(tx, point_base=pb)
    assert f"({L.DPI_ERR_UNSUPPORTED})" in str(ei.value) and "head" in str(ei.value)
    with pytest.raises(DPIError, match="Hessian"):
        gen.sample_with_gradients_and_hessians(N)
    assert _family(gen) == L.DPI_FAMILY_GENERAL  # the first-order labels of the pair run


TRAIN = """NAME: {name}
EQUATION:
  cls: Cha
  kwargs: {{nx: 10, alpha: 1.0, k: 5.0, T: 1.0}}
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
  LOSS: {{beta: 0.0, use_aux_loss: {aux}, weight_aux_loss: 0.1, SCALER: {{cls: FixedLossScaler, kwargs: {{fixed_weight: 0.1}}}}}}
  OPTIMIZER: {{kwargs: {{lr: 0.003}}}}
NETWORK:
  TYPE: {typ}
  NEURONS: [32, 32]
  ACTIVATIONS: [Tanh, Tanh]
  BOUND: None
  RELOAD: true
EVAL: {{L2_N_POINTS: 256}}
"""


@pytest.mark.parametrize("typ,aux", [(VG, True), (OG, False)])
def test_picard_train_with_a_head_net(tmp_path, typ, aux):
    """`picard train` on a small Burgers YAML (nx = 10, two Picard iterations, [32, 32]): it finishes,
    writes model_2.pt, iteration 2's labels come from the trained head net, and history.jsonl has
    finite metrics and a label throughput for both iterations."""
    from deeppicarditeration_amd.config import load_cfg
    from deeppicarditeration_amd.runner import PicardRunner
    f = tmp_path / "head.yaml"
    f.write_text(TRAIN.format(name=tmp_path / "run", typ=typ, aux=str(aux).lower()))
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
    assert seen[1][0] == "ZeroSolution" and seen[2][0] == "Sequential"
    assert all(torch.isfinite(y).all() and y.shape == (512, 11) for _, y in seen.values())
    assert not torch.equal(seen[1][1], seen[2][1])
    assert (tmp_path / "run" / "model_2.pt").exists()
    sd = torch.load(tmp_path / "run" / "model_2.pt", weights_only=True)
    assert list(sd.values())[-1].shape == (11 if typ == VG else 10,)
    recs = [json.loads(l) for l in (tmp_path / "run" / "history.jsonl").read_text().splitlines()]
    assert len(recs) == 2
    for r in recs:
        assert r["fit"] == ("head_value_gradient" if typ == VG else "head_only_gradient")
        assert r["labels_per_s"] > 0 and r["path_labels_per_s"] > 0
        for k in ("loss", "rel_l2_u", "MSE", "rRMSE", "MSEg", "rRMSEg"):
            assert np.isfinite(r[k]), (k, r[k])
