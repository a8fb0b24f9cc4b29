"""The general MLP family on GBM (csrc/dpi_general_gbm.h): first-order labels of
GBMEquationComplexExact with value nets of 1..8 hidden layers, widths <= 64, that have no specialised GBM
instance, against the fp64 oracle, and the structure around the kernel (shards, block ranges, the prepared
schedule, sampling, the estimator split, out-of-bounds writes, hipGraph capture, refusals, picard train).

Every parity case passes net_weight.gate first (tests/gbm_deep_cases.py, tests/test_gbm_deep_gates.py;
here again at the device's fp32 points without the mutants, as tests/test_gpu_network_phase.py): the
network carries 5 % .. 95 % of both blocks.  Bar: rel-L2 < 1e-4 on the value column and on the gradient
block, all labels finite, no warning inside the call, range_status() == 0, the family DPI_FAMILY_GENERAL.
Shapes: n = 3, M = 128 (two blocks per point), K = 2, nx = 7 unless the case says otherwise, seed 1, epoch 1.
Every one of these label calls raises DPIError on the parent revision (GBM: at most 3 hidden layers)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import deeppicarditeration_amd as dpi
import gbm_deep_cases as G
import net_weight as NW
from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd import data as D
from deeppicarditeration_amd._lib import DPIError
from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _case(act, widths, **kw):
    want = G._c(act, widths, **kw)
    return next(c for c in G.CASES if c == want)


def _generator(c, eq, module, M=None, K=None, **kw):
    M = c.M if M is None else M
    kw.setdefault("partial_blocks", True if M % L.DPI_PATH_BLOCK else None)
    return dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=M,
                                   n_estimate_integral=M, n_euler_steps=G.K if K is None else K, seed=G.SEED,
                                   epoch=G.EPOCH,
                                   hessian_approximation={"method": "SDGD", "kwargs": {"v": c.v}} if c.v else None, **kw)


def _setup(c, **kw):
    eq, oeq = G.equations(c)
    module, onet = G.network(c, eq, oeq)
    gen = _generator(c, eq, module, **kw)
    assert gen.net.family(gen.problem, False) == L.DPI_FAMILY_GENERAL
    return gen, oeq, onet


def _check(y, ref, what):
    parts = O.rel_l2_parts(y, ref)
    print(what, parts)
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert parts["value"] < TOL and parts["grad"] < TOL, parts


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_deep_gbm_vs_oracle(case):
    """Every case of the table; the M = 100 case runs a partial block (partial_blocks=True)."""
    c = case
    gen, oeq, onet = _setup(c)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tx, pb = gen.sample_t_and_x(G.N, point_base=0)
        y = gen.generate_with_gradients(tx, point_base=pb)
    status = gen.range_status()
    y = y.cpu().numpy()
    txh = tx.cpu().double().numpy()
    assert np.allclose(txh, O.sample_points(oeq, G.N, G.SEED, G.EPOCH, 0), rtol=0, atol=2e-5)
    info = {}
    ref = G.reference(c, oeq, onet, txh, info, with_mutants=False)  # the share band at the device's points
    parts = NW.blocks(y, ref, None)
    print(G.case_id(c), "scales", G.scales(c), "share", {k: round(v, 3) for k, v in info["share"].items()}, "rel-L2", parts)
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert status == 0
    assert all(p < TOL for p in parts.values()), parts


def test_shard_invariance():
    """label_moments over [0, 64) and [64, 128) + moments_reduce == the single call, bit for bit."""
    gen, _, _ = _setup(_case("Tanh", [64] * 4))
    tx, pb = gen.sample_t_and_x(G.N, point_base=0)
    ws = gen.point_baseline(tx)
    full = gen.label_moments(tx, pb, 128, 0, 128, L.DPI_BOTH, ws)
    parts = torch.stack([gen.label_moments(tx, pb, 128, 0, 64, L.DPI_BOTH, ws),
                         gen.label_moments(tx, pb, 128, 64, 128, L.DPI_BOTH, ws)]).contiguous()
    assert torch.isfinite(full).all() and torch.equal(gen.moments_reduce(parts), full)


def test_block_ranges():
    """4 points x 1,024 blocks = 4,096 blocks, 16 launches of 256-block ranges on the stash's slots, more
    than 64 blocks per point (the k_reduce launch, not the fused reduce): point 0 against the oracle, and
    the whole call bit-identical to four one-point calls."""
    n, M = 4, 65536
    c = _case("ELU", [16] * 5, v=7)
    gen, oeq, onet = _setup(c, M=M, K=1)
    slots = gen.net.general_slots()
    assert slots > 0 and n * (M // 64) > 2 * slots
    tx, pb = gen.sample_t_and_x(n, point_base=0)
    y = gen.generate_with_gradients(tx, point_base=pb)
    ref = O.labels_grad(oeq, onet, tx[:1].cpu().double().numpy(), M, 1, G.SEED, G.EPOCH, pb, v=c.v)
    _check(y[:1].cpu().numpy(), ref, "block ranges, point 0")
    for i in range(n):
        yi = gen.generate_with_gradients(tx[i:i + 1].contiguous(), point_base=pb + i)
        assert torch.equal(yi, y[i:i + 1]), i


def test_prepared_call_is_bitwise_the_plain_call():
    """dpi_label_prepare (k_noise_shared's staged noise sums) + DPI_PREPARED == the plain call."""
    gen, _, _ = _setup(_case("ELU", [64] * 8, v=7))
    tx, pb = gen.sample_t_and_x(G.N, point_base=0)
    ws = D.new_workspace(gen.workspace_bytes(G.N, 128, prepared=True), "cuda:0")
    gen.point_baseline(tx, ws=ws)
    plain = gen.label_moments(tx, pb, 128, 0, 128, L.DPI_BOTH, ws)
    gen.label_prepare(tx, pb, 128, 0, 128, L.DPI_BOTH, ws)
    prepared = gen.label_moments(tx, pb, 128, 0, 128, L.DPI_BOTH | L.DPI_PREPARED, ws)
    torch.cuda.synchronize()
    assert torch.isfinite(plain).all() and torch.equal(plain, prepared)


def test_sharded_labeler_prepare_equals_labels():
    """ShardedLabeler.prepare -> begin -> end, one batch in flight, against labels() on the same points."""
    from deeppicarditeration_amd.sharding import ShardedLabeler
    c = _case("Tanh", [64] * 4)
    lab, ref = ShardedLabeler(_setup(c)[0]), ShardedLabeler(_setup(c)[0])
    got, pending = [], []
    for _ in range(3):
        pending.append(lab.begin(prepared=lab.prepare(5)))
        if len(pending) > 1:
            got.append(lab.end(pending.pop(0)))
    got.append(lab.end(pending.pop(0)))
    torch.cuda.synchronize()
    for y in got:
        tx, pb = ref.gen.sample_t_and_x(5)
        assert torch.isfinite(y).all() and torch.equal(y, ref.labels(tx, pb))


def test_sample_with_gradients_equals_its_two_calls():
    c = _case("ELU", [32] * 4, v=7)
    a, b = _setup(c)[0], _setup(c)[0]
    tx, y = a.sample_with_gradients(G.N)
    tx2, pb = b.sample_t_and_x(G.N, point_base=0)
    y2 = b.generate_with_gradients(tx2, point_base=pb)
    assert torch.equal(tx, tx2) and torch.isfinite(y).all() and torch.equal(y, y2)


def test_estimator_split():
    c = _case("Tanh", [40], v=7)
    gen, oeq, onet = _setup(c)
    tx, pb = gen.sample_t_and_x(G.N, point_base=0)
    yT = gen.estimate_terminal_with_gradients(tx, point_base=pb).cpu().numpy()
    yI = gen.estimate_integral_with_gradients(tx, point_base=pb).cpu().numpy()
    _, rT, rI = O.labels_grad(oeq, onet, tx.cpu().double().numpy(), c.M, G.K, G.SEED, G.EPOCH, pb, v=c.v,
                              return_parts=True)
    _check(yT, rT, "terminal only")
    _check(yI, rI, "integral only")


def test_canary():
    """8 x 64 at nx = 128, M = 100 (a partial block; the LDS and stash worst case): nothing is written past
    the workspace (whose last region is the stash), the moments or the labels."""
    from test_gpu_canary import Carved, _stream
    nx, n, M = 128, 3, 100
    eq, _ = G.equations(G._c("ELU", [64] * 8, nx=nx))
    torch.manual_seed(17)
    gen = _generator(G._c("ELU", [64] * 8, nx=nx, v=7), eq, dpi.construct_mlp(1 + nx, 1, [64] * 8, ["ELU"] * 8, None),
                     M=M)
    assert gen.net.family(gen.problem, False) == L.DPI_FAMILY_GENERAL
    F = 1 + nx
    c = Carved(ws=gen.workspace_bytes(n, M), mom=n * 2 * F * 4, y=n * F * 4)
    tx, pb = gen.sample_t_and_x(n, point_base=11)
    gen.point_baseline(tx, ws=c.u8("ws"))
    args = (gen.problem, gen.net.handle, ctypes.c_void_p(tx.data_ptr()), n, M, gen.K, gen.seed, gen.epoch, pb)
    L.check(gen.lib.dpi_label_moments_finalize(*args, L.DPI_BOTH, float("inf"), c.ptr("y"), c.ptr("mom"), c.ptr("ws"),
                                               c.nbytes("ws"), _stream()), "moments_finalize")
    c.check()
    assert torch.isfinite(c.f32("mom", n, 2, F)).all() and torch.isfinite(c.f32("y", n, F)).all()


def test_label_call_captures_into_a_hip_graph():
    """A whole label call (baseline, path launch, reduce, finalize) captured and replayed: the eager labels."""
    gen, _, _ = _setup(_case("ELU", [64] * 4))
    tx, _ = gen.sample_t_and_x(6, point_base=40)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = gen.generate_with_gradients(tx, point_base=40).clone()  # also sizes the workspace before capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = gen.generate_with_gradients(tx, point_base=40)
    for _ in range(2):
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(y).all() and torch.equal(y, eager)


def _plain(nx, widths, **kw):
    eq, _ = G.equations(G._c("ELU", widths, nx=nx))
    torch.manual_seed(17)
    module = dpi.construct_mlp(1 + nx, 1, list(widths), ["ELU"] * len(widths), None)
    return _generator(G._c("ELU", widths, nx=nx), eq, module, **kw)


@pytest.mark.parametrize("widths", [[65], [64, 128]], ids=["65", "64x128"])
def test_wider_than_64_is_refused_by_name(widths):
    gen = _plain(7, widths)
    with pytest.raises(DPIError, match="GBM") as ei:
        gen.generate_with_gradients(*gen.sample_t_and_x(G.N, point_base=0))
    assert f"({L.DPI_ERR_UNSUPPORTED})" in str(ei.value) and "64" in str(ei.value)
    with pytest.raises(DPIError, match="GBM"):
        gen.net.family(gen.problem, False)


@pytest.mark.parametrize("what", ["td", "hessian", "nx129"])
def test_out_of_scope_pairs_are_refused_by_name(what):
    """TD estimators, Hessian labels and nx > 128 of a pair the new family serves: DPI_ERR_UNSUPPORTED naming
    the cap, at the label call and (TD, nx: its arguments) from dpi_pair_family."""
    gen = _plain(129 if what == "nx129" else 7, [64] * 4, estimate_delta_t=0.3 if what == "td" else None)
    word = {"td": "TD", "hessian": "Hessian", "nx129": "128"}[what]
    call = gen.generate_with_gradients_and_hessians if what == "hessian" else gen.generate_with_gradients
    with pytest.raises(DPIError, match=word) as ei:
        call(*gen.sample_t_and_x(G.N, point_base=0))
    assert f"({L.DPI_ERR_UNSUPPORTED})" in str(ei.value)
    if what == "hessian":  # dpi_pair_family has no Hessian argument: the pair itself is served
        assert gen.net.family(gen.problem, False) == L.DPI_FAMILY_GENERAL
    else:
        with pytest.raises(DPIError, match=word):
            gen.net.family(gen.problem, what == "td")


TRAIN = """NAME: {name}
EQUATION:
  cls: GBMEquationComplexExact
  kwargs: {{nx: 8, alpha: 1.0, T: 1.0, w: {w}, v: {v}}}
PICARD: {{N: 2}}
FORCE: true
DATA:
  DATA_SIZE: 512
  POINTS_PER_CALL: 256
  EULER_STEPS: 4
  HESSIAN_APPROXIMATION: {{method: SDGD, kwargs: {{v: 4}}}}
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
    """`picard train` on GBM with NETWORK.NEURONS [24] * 5 and SDGD: iteration 2's labels come from the
    trained five-layer iterate through the new family; the Hessian labels TRAIN.SUPERVISE_HESSIAN would ask
    of that iterate are refused by name."""
    from deeppicarditeration_amd.config import load_cfg
    from deeppicarditeration_amd.runner import PicardRunner
    rng = np.random.default_rng(8)
    w = rng.standard_normal((2, 9)) / np.sqrt(8)
    w[:, 0] = 1.0
    f = tmp_path / "gbm5.yaml"
    f.write_text(TRAIN.format(name=tmp_path / "run", w=w.tolist(), v=rng.standard_normal((2, 1)).tolist()))
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
    gen = runner.make_generator(runner.u_current)
    assert gen.net.family(gen.problem, False) == L.DPI_FAMILY_GENERAL
    with pytest.raises(DPIError, match="Hessian"):
        gen.sample_with_gradients_and_hessians(4)
