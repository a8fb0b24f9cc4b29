"""Monte-Carlo sample counts that are no multiple of the 64-path block, on the GPU.

A label call over [m_begin, m_end) of M launches ceil((m_end - m_begin) / 64) workgroups per point;
the lanes of the last one with m >= m_end are dead: they roll out and evaluate like any other and
add exactly +0 to every sum (include/dpi.h dpi_label_moments).  Every case here is checked against
the fp64 oracle (oracle/dpi_oracle.py, which takes any count) or bitwise against another form of the
same call.

Shapes: those of tests/test_gpu_dispatch_rows.py (n = 3 points, K = 2, nx = 7 narrow / 129 wide, TD
at 0.3), PISGradNet [32, 32] at nx = 100 with n = 2.  M = 100 is one full block and a 36-lane tail,
so the cross-block reduce runs; 1, 63 and 65 are the single lane, the single dead lane and the
single live lane of a tail.  Tolerance: the suite's rel-L2 < 1e-4 per block of the label, all
outputs finite.  A kernel that forgets the mask — the sum over ceil64(M) paths divided by M — is
at least 3.7e-3 from the oracle at these shapes (Cha at M = 63), so it cannot pass."""
import functools
import json
import warnings

import numpy as np
import pytest
import torch

import deeppicarditeration_amd as dpi
from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd import data as D
from golden_util import delta_t, load, m_terminal
from gpu_util import product_equation, product_module
from oracle import dpi_oracle as O
from test_gpu_dispatch_rows import CASES, DT, EPOCH, K, N, SEED, _equation, _net

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _gen(eq, module, MT, MI, k=K, dt=0.0, seed=SEED, epoch=EPOCH, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", D.PartialBlockNote)
        return dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=MT,
                                       n_estimate_integral=MI, n_euler_steps=k, seed=seed, epoch=epoch,
                                       estimate_delta_t=dt if dt else None, partial_blocks=True, **kw)


class _mode:
    """The process-wide GEMM mode for the nets named *-f32 (exact fp32) or otherwise (the default)."""

    def __init__(self, f32):
        self.f32 = f32

    def __enter__(self):
        L.check(L.load().dpi_set_gemm_precision(L.DPI_GEMM_F32 if self.f32 else L.DPI_GEMM_AUTO), "gemm precision")

    def __exit__(self, *a):
        L.check(L.load().dpi_set_gemm_precision(L.DPI_GEMM_AUTO), "gemm precision")


def _check(y, ref, nx, what):
    y = np.asarray(y, np.float64)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert np.isfinite(y).all(), what
    blocks = {"value": slice(0, 1), "grad": slice(1, 1 + nx)}
    if y.shape[1] > 1 + nx:
        blocks["hess"] = slice(1 + nx, None)
    err = {k: O.rel_l2(y[:, sl], ref[:, sl]) for k, sl in blocks.items()}
    print(what, err)
    assert all(e < TOL for e in err.values()), (what, err)


def _points(tx):
    """The GPU's fp32 points as a hashable key of the cached references (the draws do not depend on
    the net or the GEMM mode, so the modes of one net share a reference)."""
    tx = np.ascontiguousarray(tx.detach().cpu().double().numpy())
    return tx.shape, tx.tobytes()


def _unkey(key):
    return np.frombuffer(key[1], np.float64).reshape(key[0])


@functools.lru_cache(maxsize=None)
def _first_order_reference(eq_kind, act, variant, net, MT, MI, key):
    """The oracle's labels for a unit-table row at the GPU's points, computed once per (row, net
    shape, counts); the fused-baseline rows draw their points themselves: (tx, labels)."""
    nx = 129 if variant == "wide" else 7
    eq, oeq = _equation(eq_kind, nx)
    _, onet = _net(eq, net, act)
    if variant == "fb":
        assert MT == MI
        return O.sample_with_gradients(oeq, onet, N, MI, K, SEED, EPOCH, 0)
    tx = _unkey(key)
    return tx, O.labels_grad(oeq, onet, tx, MI, K, SEED, EPOCH, 0, delta_t=DT if variant == "td" else 0.0, MT=MT)


def _run_row(eq_kind, act, variant, net, MT, MI):
    nx = 129 if variant == "wide" else 7
    dt = DT if variant == "td" else 0.0
    eq, _ = _equation(eq_kind, nx)
    module, _ = _net(eq, net, act)
    with _mode(net.endswith("f32")):
        gen = _gen(eq, module, MT, MI, dt=dt)
        if variant == "fb":  # points and labels in one call
            tx, y = gen.sample_with_gradients(N)
        else:
            tx, pb = gen.sample_t_and_x(N, point_base=0)
            y = gen.generate_with_gradients(tx, point_base=pb)
        y = y.cpu().numpy()
    shape = net.replace("-f32", "").replace("-auto", "")
    otx, ref = _first_order_reference(eq_kind, act, variant, shape, MT, MI, None if variant == "fb" else _points(tx))
    assert np.allclose(tx.cpu().numpy(), otx, rtol=0, atol=2e-5)
    _check(y, ref, nx, (eq_kind, act, variant, net, MT, MI))


# ---- 1. every unit-table row x net at M = 100
@pytest.mark.parametrize("eq_kind,act,variant,net", CASES, ids=["-".join(c) for c in CASES])
def test_unit_rows_at_100_paths(eq_kind, act, variant, net):
    _run_row(eq_kind, act, variant, net, 100, 100)


# ---- 2. the single lane, the single dead lane, the single live lane of a tail
EDGE_ROWS = [("cha", "ELU", "plain"), ("gbm", "ELU", "plain"), ("ou", "ELU", "td"), ("cha", "ELU", "wide"),
             ("cha", "ELU", "fb")]


@pytest.mark.parametrize("M", [1, 63, 65])
@pytest.mark.parametrize("net", ["w32x2-auto", "zero"])
@pytest.mark.parametrize("row", EDGE_ROWS, ids=["-".join(r) for r in EDGE_ROWS])
def test_edge_counts(row, net, M):
    _run_row(*row, net, M, M)


# ---- 2b. the split OU 4 x 128 instance forms its mask from the block's live-lane count (dpi_device.h
# MASK_SCALAR), every other instance from m < m_end: the same cases on that instance
def _ou128():
    eq, oeq = _equation("ou", 7)
    torch.manual_seed(17)
    m = dpi.construct_mlp(8, 1, [128] * 4, ["ELU"] * 4, None)
    lin = [l for l in m if isinstance(l, torch.nn.Linear)]
    onet = O.MLP([l.weight.detach().double().numpy() for l in lin], [l.bias.detach().double().numpy() for l in lin],
                 ["ELU"] * 4)
    return eq, oeq, m, onet


@pytest.mark.parametrize("M", [1, 65, 100])
def test_split_ou_4x128_instance(M):
    eq, oeq, module, onet = _ou128()
    gen = _gen(eq, module, M, M)  # the default (fp16-split) mode
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    y = gen.generate_with_gradients(tx, point_base=pb).cpu().numpy()
    ref = O.labels_grad(oeq, onet, tx.cpu().double().numpy(), M, K, SEED, EPOCH, 0)
    _check(y, ref, 7, ("ou 4x128 split", M))


# ---- 3. unequal estimator counts
@pytest.mark.parametrize("MT,MI", [(37, 100), (100, 1)])
@pytest.mark.parametrize("eq_kind", ["cha", "gbm"])
def test_unequal_counts(eq_kind, MT, MI):
    _run_row(eq_kind, "ELU", "plain", "w32x2-auto", MT, MI)


# ---- 4. Hessian labels
@functools.lru_cache(maxsize=None)
def _hessian_reference(net, MT, MI, key):
    eq, oeq = _equation("gbm", 7)
    _, onet = _net(eq, net, "ELU")
    return O.labels_grad_hess(oeq, onet, _unkey(key), MI, K, SEED, EPOCH, 0, MT=MT)


@pytest.mark.parametrize("MT,MI", [(1, 1), (100, 100), (37, 100)])
@pytest.mark.parametrize("net", ["w32x2-f32", "w32x2-auto", "zero"])
def test_hessian_labels(net, MT, MI):
    eq, _ = _equation("gbm", 7)
    module, _ = _net(eq, net, "ELU")
    with _mode(net.endswith("f32")):
        gen = _gen(eq, module, MT, MI)
        tx, pb = gen.sample_t_and_x(N, point_base=0)
        y = gen.generate_with_gradients_and_hessians(tx, point_base=pb).cpu().numpy()
    ref = _hessian_reference(net.replace("-f32", "").replace("-auto", ""), MT, MI, _points(tx))
    _check(y, ref, 7, ("gbm hess", net, MT, MI))
    h = y[:, 8:].reshape(N, 7, 7)
    assert np.array_equal(h, np.transpose(h, (0, 2, 1)))


# ---- 5. PISGradNet
def _pis():
    eq = dpi.OUProcessEquation(nx=100, T=1.0, alpha=1.0, num_components=5, mean_scale=1.0, var_scale=2.0,
                               alpha_scale=4.0)
    torch.manual_seed(5)
    net = dpi.PISGradNet(hidden_shapes=[32, 32], dim=100, g0=eq.g, T=1.0)
    with torch.no_grad():
        net.timestep_phase.copy_(0.1 * torch.randn(1, 64))
    return eq, net


@functools.lru_cache(maxsize=None)
def _pis_reference(M, dt, key):
    eq, net = _pis()
    oeq = O.OUProcessEquation(100, eq.mean.numpy(), eq.var.numpy(), eq.pi.numpy(), alpha_scale=4.0)
    onet = O.PISGradNet({k: v.detach().double().numpy() for k, v in net.state_dict().items()}, oeq, T=1.0)
    return O.labels_grad(oeq, onet, _unkey(key), M, K, SEED, EPOCH, 0, delta_t=dt)


@pytest.mark.parametrize("M,dt", [(1, 0.0), (65, 0.0), (65, 0.55)], ids=["M1", "M65", "M65-td"])
@pytest.mark.parametrize("gemm", ["auto", "f32"])
def test_pisgradnet(gemm, M, dt):
    eq, net = _pis()
    with _mode(gemm == "f32"):
        gen = _gen(eq, net, M, M, dt=dt)
        tx, pb = gen.sample_t_and_x(2, point_base=0)
        if dt:
            t = tx[:, 0].cpu().numpy()
            assert (t + dt < 1).any() and (t + dt >= 1).any()
        y = gen.generate_with_gradients(tx, point_base=pb).cpu().numpy()
    _check(y, _pis_reference(M, dt, _points(tx)), 100, ("pis", gemm, M, dt))


@pytest.mark.parametrize("gemm", ["auto", "f32"])
def test_pisgradnet_prepared_call_is_bitwise_the_plain_call(gemm):
    eq, net = _pis()
    with _mode(gemm == "f32"):
        gen = _gen(eq, net, 100, 100)
        tx, pb = gen.sample_t_and_x(2, point_base=0)
        ws = D.new_workspace(gen.workspace_bytes(2, 100, prepared=True), "cuda:0")
        gen.point_baseline(tx, ws=ws)
        plain = gen.label_moments(tx, pb, 100, 0, 100, L.DPI_BOTH, ws)
        gen.label_prepare(tx, pb, 100, 0, 100, L.DPI_BOTH, ws)
        prepared = gen.label_moments(tx, pb, 100, 0, 100, L.DPI_BOTH | L.DPI_PREPARED, ws)
        torch.cuda.synchronize()
    assert torch.isfinite(plain).all() and torch.equal(plain, prepared)


# ---- 6. the reference-made fixtures, both MFMA modes
PARTIAL = ["cha_mlp16_M100_K2", "cha_mlp16_M1_K2", "ou_pis32_M65_K2", "gbm_mlp32x3_M100_MT37_K2",
           "gbm_hess_mlp32x3_M100_K2"]


@pytest.mark.parametrize("gemm", ["auto", "f32"])
@pytest.mark.parametrize("case", PARTIAL)
def test_reference_fixtures(case, gemm):
    f = load(f"partial/{case}")
    eq = product_equation(f)
    module = product_module(f, eq)
    with _mode(gemm == "f32"):
        gen = _gen(eq, module, m_terminal(f), int(f["M"]), k=int(f["K"]), dt=delta_t(f), seed=int(f["seed"]),
                   epoch=int(f["epoch"]))
        tx = torch.as_tensor(f["tx"], dtype=torch.float32, device="cuda:0")
        call = gen.generate_with_gradients_and_hessians if bool(f["hessians"]) else gen.generate_with_gradients
        y = call(tx, point_base=int(f["point_base"])).cpu().numpy()
    _check(y, f["y"], eq.nx, (case, gemm))


# ---- 7. bitwise invariants at M = 100
def _cha_gen(M=100):
    eq, _ = _equation("cha", 7)
    module, _ = _net(eq, "w32x2-auto", "ELU")
    return _gen(eq, module, M, M)


def test_two_ranges_combine_to_the_single_call():
    gen = _cha_gen()
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ws = gen.point_baseline(tx)
    one = gen.label_moments(tx, pb, 100, 0, 100, L.DPI_BOTH, ws)
    parts = torch.stack([gen.label_moments(tx, pb, 100, 0, 64, L.DPI_BOTH, ws),
                         gen.label_moments(tx, pb, 100, 64, 100, L.DPI_BOTH, ws)])
    two = gen.moments_reduce(parts)
    torch.cuda.synchronize()
    assert torch.isfinite(one).all() and torch.equal(one, two)
    with pytest.raises(L.DPIError, match="multiple of 64"):  # a range that ends inside a block before M
        gen.label_moments(tx, pb, 100, 0, 36, L.DPI_BOTH, ws)


def test_one_launch_form_equals_two_launches_and_the_separate_reduce(monkeypatch):
    gen = _cha_gen()
    monkeypatch.setenv("DPI_FUSED_REDUCE", "1")
    monkeypatch.setenv("DPI_FUSED_BASE", "1")
    tx1, y1 = gen.sample_generate(N, 0)
    mom1 = gen.last_moments
    monkeypatch.setenv("DPI_FUSED_BASE", "0")
    tx2, y2 = gen.sample_generate(N, 0)
    mom2 = gen.last_moments
    monkeypatch.setenv("DPI_FUSED_REDUCE", "0")
    tx3, y3 = gen.sample_generate(N, 0)
    mom3 = gen.last_moments
    torch.cuda.synchronize()
    assert torch.isfinite(y1).all()
    assert torch.equal(tx1, tx2) and torch.equal(y1, y2) and torch.equal(mom1, mom2)
    assert torch.equal(tx1, tx3) and torch.equal(y1, y3) and torch.equal(mom1, mom3)


@pytest.mark.parametrize("hessians", [False, True])
def test_gbm_prepared_call_is_bitwise_the_plain_call(hessians):
    eq, _ = _equation("gbm", 7)
    module, _ = _net(eq, "w32x2-auto", "ELU")
    gen = _gen(eq, module, 100, 100)
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ws = D.new_workspace(gen.workspace_bytes(N, 100, hessians=hessians, prepared=True), "cuda:0")
    gen.point_baseline(tx, hessians=hessians, ws=ws)
    if hessians:
        def call(flags):
            return gen.label_moments_hessians(tx, pb, 100, 0, 100, ws, flags=flags)
    else:
        def call(flags):
            return (gen.label_moments(tx, pb, 100, 0, 100, flags, ws),)
    plain = call(L.DPI_BOTH)
    gen.label_prepare(tx, pb, 100, 0, 100, L.DPI_BOTH, ws)
    prepared = call(L.DPI_BOTH | L.DPI_PREPARED)
    torch.cuda.synchronize()
    for a, b in zip(plain, prepared):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- 8. more paths than one call takes, the second call a ragged tail
def test_two_calls_with_a_ragged_tail():
    M = 65536 + 37
    eq, oeq = _equation("cha", 7)
    gen = _gen(eq, dpi.ZeroSolution(1), M, M, k=1)
    tx, pb = gen.sample_t_and_x(1, point_base=0)
    assert gen._pieces(0, M) == [(0, 65536), (65536, M)]
    y = gen.generate_with_gradients(tx, point_base=pb).cpu().numpy()
    ref = O.labels_grad(oeq, O.ZeroNet(), tx.cpu().double().numpy(), M, 1, SEED, EPOCH, 0, m_chunk=8192)
    _check(y, ref, 7, ("cha zero", M))


# ---- 9. the constructor's opt-in and its note
def test_constructor_opt_in_and_note(monkeypatch):
    monkeypatch.setattr(D, "_PARTIAL_NOTED", set())
    eq = dpi.Cha(7, 1.0, 5.0, 1.0)

    def make(M, **kw):
        return dpi.OnlineDataGenerator(eq, dpi.ZeroSolution(1), 1, 1, device="cuda:0", t_always_uniform=True,
                                       n_estimate_terminal=M, n_estimate_integral=M, n_euler_steps=2, **kw)

    with pytest.raises(ValueError):
        make(100)
    with pytest.raises(ValueError):
        make(100, partial_blocks=False)
    with pytest.raises(ValueError):
        make(0, partial_blocks=True)
    for M in (100, 64):
        with warnings.catch_warnings():
            warnings.simplefilter("error", D.PartialBlockNote)
            assert make(M, partial_blocks=True).n_estimate_integral == M
    for M in (1, 20):
        with pytest.warns(D.PartialBlockNote, match="64"):
            assert make(M, partial_blocks=True).n_estimate_terminal == M
        with warnings.catch_warnings():  # once per (class, M)
            warnings.simplefilter("error", D.PartialBlockNote)
            make(M, partial_blocks=True)
    assert issubclass(D.PartialBlockNote, UserWarning)

    # a class default stands in for the keyword (the reference binding derives such a class)
    from deeppicarditeration_amd.picard_binding import generator_class

    class Base:
        pass

    cls = generator_class(Base)
    assert cls.partial_blocks_default is True and dpi.OnlineDataGenerator.partial_blocks_default is False
    g = cls(eq, dpi.ZeroSolution(1), 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=100,
            n_estimate_integral=100, n_euler_steps=2)
    tx, y = g.sample_with_gradients(2)
    assert torch.isfinite(y).all()


@pytest.mark.parametrize("with_base", [False, True])
def test_binding_takes_the_reference_counts(with_base):
    """picard_binding.hip_online_data_generator, the call the patched data module makes: the `kws` it
    forwards hold the reference's counts (100, and the constructor default of 1 when DATA.kwargs
    leaves them out), with the reference's base class or without one."""
    from deeppicarditeration_amd.picard_binding import hip_online_data_generator

    class Base:
        pass

    eq = dpi.Cha(7, 1.0, 5.0, 1.0)
    for counts in ({"n_estimate_terminal": 100, "n_estimate_integral": 100}, {}):
        kws = dict(equation=eq, solution=dpi.ZeroSolution(1), N=1, i=1, device="cuda:0", t_always_uniform=True,
                   **counts)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", D.PartialBlockNote)
            gen = hip_online_data_generator(kws, {"EULER_STEPS": 2, "SEED": 3}, base=Base if with_base else None)
        assert isinstance(gen, dpi.OnlineDataGenerator) and (not with_base or isinstance(gen, Base))
        assert gen.n_estimate_integral == counts.get("n_estimate_integral", 1)
        tx, y = gen.sample_with_gradients(2)
        assert y.shape == (2, 8) and torch.isfinite(y).all()


# ---- 10. picard train with the reference's default sample counts
BURGERS_DEFAULT_COUNTS = """NAME: {name}
EQUATION:
  cls: Cha
  kwargs: {{nx: 100, alpha: 1.0, k: 5.0, T: 1.0}}
PICARD: {{N: 2}}
FORCE: true
DATA:
  FLOAT: float
  DATA_SIZE: 256
  POINTS_PER_CALL: 128
  SEED: 5
  kwargs: {{t_always_uniform: true}}
TRAIN:
  N_EPOCHS: 2
  BATCH_SIZE: 64
  SUPERVISE_GRADIENT: true
  LOSS: {{beta: 0.0, SCALER: {{cls: FixedLossScaler, kwargs: {{fixed_weight: 0.0}}}}}}
NETWORK:
  NEURONS: [128, 128, 128, 128]
  ACTIVATIONS: ["ELU", "ELU", "ELU", "ELU"]
  BOUND: None
  RELOAD: true
EVAL: {{L2_N_POINTS: 100, TEST_GRAD: true}}
"""


def test_picard_train_with_the_default_sample_counts(tmp_path):
    """The Burgers YAML (scripts/burgers/base_100d_T1.0_w0.0_0.yaml's keys) with n_estimate_* left to
    the constructor default of 1, as the reference takes it: two Picard iterations on the device
    path, finite labels, a history record each."""
    from deeppicarditeration_amd.config import load_cfg
    from deeppicarditeration_amd.runner import PicardRunner
    f = tmp_path / "burgers.yaml"
    f.write_text(BURGERS_DEFAULT_COUNTS.format(name=tmp_path / "run"))
    runner = PicardRunner(load_cfg(str(f)))
    assert "n_estimate_integral" not in dict(runner.cfg.DATA.kwargs)
    seen = {}
    orig = runner.labels

    def labels():
        tx, y = orig()
        seen[runner.i] = (tx, y)
        return tx, y

    runner.labels = labels
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", D.PartialBlockNote)
        gen = runner.make_generator(runner.u_current)
        assert gen.n_estimate_terminal == 1 and gen.n_estimate_integral == 1
        hist = runner.run()
    assert [h["iter"] for h in hist] == [1, 2] and all(h["labels"] == 256 for h in hist)
    for i in (1, 2):
        tx, y = seen[i]
        assert y.shape == (256, 101) and torch.isfinite(y).all() and torch.isfinite(tx).all()
    assert all(h["loss"] == h["loss"] for h in hist)
    lines = (tmp_path / "run" / "history.jsonl").read_text().splitlines()
    assert [json.loads(l)["iter"] for l in lines] == [1, 2]
