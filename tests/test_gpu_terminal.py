"""Terminal-enforcing solutions (NETWORK.cls PicardSolutionEnforceTerminal; csrc/dpi_general.h TERMA,
DESIGN.md §2.16) on the GPU: u = g + (T - t) N for a Value net and grad u = grad g + (T - t) N, u = 0, for
an OnlyGradient net, first-order Cha / OU labels in the general MLP family — against the fp64 oracle
(oracle/dpi_oracle.py) with the wrapper's twin (tests/terminal_util.py TerminalNet) and against the
reference's own labels (tests/golden/terminal/*.npz).

Shapes as tests/test_gpu_general_mlp.py: n = 3 points, M = 128 paths (two 64-path blocks per point, so
the cross-block reduce runs), K = 2 Euler steps, seed 1, epoch 1; nx = 7 (the padding lanes are live),
100 and 128.  Tolerance: the suite's rel-L2 < 1e-4 on the value column and on the gradient block; all
labels finite, range_status() == 0.

Nets: tests/terminal_util.py scaled_mlp (torch.manual_seed(17), construct_mlp, scaled by SCALES).  Every
oracle case first asserts on the CPU, at the case's own points, that the ansatz matters (gate (a)) and
that the net matters (gate (b)); tests/test_terminal_gates.py holds the same gates without a GPU."""
import ctypes
import json

import numpy as np
import pytest
import torch

import deeppicarditeration_amd as dpi
import terminal_util as T
from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd._lib import DPIError
from deeppicarditeration_amd.solution import PicardSolutionEnforceTerminal
from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
N, M, K, SEED, EPOCH = T.N, T.M, T.K, T.SEED, T.EPOCH
V, OG = "Value", "OnlyGradient"


def _gen(eq, module, M_=M, K_=K, **kw):
    return dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=M_,
                                   n_estimate_integral=M_, n_euler_steps=K_, seed=SEED, epoch=EPOCH, **kw)


def _case(eq_kind, kind, act, wtag, nx):
    """(equation, oracle equation, wrapper module, oracle twin)."""
    eq, oeq = T.equation(eq_kind, nx)
    inner, acts = T.case_nets(eq_kind, kind, act, wtag, nx)
    return eq, oeq, PicardSolutionEnforceTerminal(eq, inner, kind), T.from_module(oeq, inner, acts, kind)


def _family(gen, td=False):
    return gen.net.family(gen.problem, td)


def _gated_ref(oeq, twin, txh, M_=M, K_=K, pb=0, what=""):
    ref, a, b = T.gate_parts(oeq, twin, txh, M_, K_, pb)
    T.assert_gates(a, b, what)
    return ref


def _check(y, ref, what):
    parts = O.rel_l2_parts(y, ref)
    print(what, parts)
    assert np.isfinite(y).all()
    assert parts["value"] < TOL and parts["grad"] < TOL, parts


def _is_terminal(gen, kind):
    assert _family(gen) == L.DPI_FAMILY_GENERAL
    assert gen.net.desc.endswith(f"-{kind}-terminal"), gen.net.desc
    assert (gen.net.general_slots() > 0) == (kind == V)


# ------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("case", T.GPU_CASES, ids=T.case_id)
def test_terminal_net_vs_oracle(case):
    eq_kind, kind, act, wtag, nx = case
    eq, oeq, module, twin = _case(*case)
    gen = _gen(eq, module)
    _is_terminal(gen, kind)  # [128] * 4 too: general, not the specialised fp16-split kernels
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ref = _gated_ref(oeq, twin, tx.cpu().double().numpy(), what=T.case_id(case))
    y = gen.generate_with_gradients(tx, point_base=pb).cpu().numpy()
    _check(y, ref, T.case_id(case))
    assert gen.range_status() == 0


@pytest.mark.parametrize("name", T.TERMINAL_CASES)
def test_golden_reference_parity(name):
    """The reference's own labels of its own class, on the same noise."""
    from gpu_util import generator, product_equation
    f = T.load(name)
    eq = product_equation(f)
    kind, neurons = str(f["type"]), [int(v) for v in f["neurons"]]
    inner = dpi.construct_mlp(1 + eq.nx, 1 if kind == V else eq.nx, neurons, [str(a) for a in f["acts"]], None)
    inner.load_state_dict({k[3:]: torch.as_tensor(v).float() for k, v in f.items() if k.startswith("sd_")})
    f = {**f, "v": 0}
    gen = generator(f, eq, PicardSolutionEnforceTerminal(eq, inner, kind))
    _is_terminal(gen, kind)
    tx = torch.as_tensor(f["tx"], dtype=torch.float32, device="cuda:0")
    y = gen.generate_with_gradients(tx, point_base=int(f["point_base"])).cpu().numpy()
    _check(y, f["y"], name)
    assert gen.range_status() == 0


# ------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("eq_kind,kind", [("cha", V), ("ou", V), ("cha", OG), ("ou", OG)])
def test_hand_made_points_at_both_ends_of_time(eq_kind, kind):
    """t = 0 (T - s spans the whole horizon) and t = T - 1e-3 (T - s is tiny on every path, u -> g): T - s
    is formed as (T - t)(1 - U), not as T - fl(s).  The early rows pass both gates.  At the late rows the
    integral term carries the factor T - t = 1e-3 and the label is the terminal estimator's, which the
    network does not enter: the net cannot matter, and the ansatz moves the label by 2.5e-3 .. 3e-2 only
    (fp64 oracle).  What is asserted there is that labels without g and grad g are at least 10 x the parity
    bar away, so the parity check that follows would catch their loss."""
    nx = 7
    eq, oeq, module, twin = _case(eq_kind, kind, "ELU", "w64x4", nx)
    gen = _gen(eq, module)
    x = O.sample_points(oeq, 4, SEED, EPOCH, 0)[:, 1:]
    txh = np.concatenate([np.array([[0.0], [0.0], [1.0 - 1e-3], [1.0 - 1e-3]]), x], 1).astype(np.float32)
    tx = torch.as_tensor(txh, device="cuda:0")
    y = gen.generate_with_gradients(tx, point_base=0).cpu().numpy()
    txd = txh.astype(np.float64)
    early, late = slice(0, 2), slice(2, 4)
    ref = _gated_ref(oeq, twin, txd[early], what="t = 0")
    _check(y[early], ref, (eq_kind, kind, "t = 0"))
    ref_late, a, _ = T.gate_parts(oeq, twin, txd[late], M, K, late.start)
    assert a["value"] >= 10 * TOL and a["grad"] >= 10 * TOL, ("the ansatz at t = T - 1e-3", a)
    _check(y[late], ref_late, (eq_kind, kind, "t = T - 1e-3"))
    assert gen.range_status() == 0


@pytest.mark.parametrize("eq_kind,kind", [("ou", V), ("cha", OG)])
def test_partial_block(eq_kind, kind):
    """M = 100: the second block of every point has 36 live lanes."""
    eq, oeq, module, twin = _case(eq_kind, kind, "ELU", "w128x4", 7)
    gen = _gen(eq, module, M_=100, partial_blocks=True)
    _is_terminal(gen, kind)
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ref = _gated_ref(oeq, twin, tx.cpu().double().numpy(), 100, K)
    _check(gen.generate_with_gradients(tx, point_base=pb).cpu().numpy(), ref, "partial block")


@pytest.mark.parametrize("eq_kind,kind", [("ou", V), ("cha", V), ("ou", OG)])
def test_shard_invariance(eq_kind, kind):
    """label_moments over [0, 64) and [64, 128) + moments_reduce == the single call, bit for bit."""
    eq, _, module, _ = _case(eq_kind, kind, "Tanh", "w256x2", 7)
    gen = _gen(eq, module)
    _is_terminal(gen, kind)
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ws = gen.point_baseline(tx)
    full = gen.label_moments(tx, pb, M, 0, M, L.DPI_BOTH, ws)
    parts = torch.stack([gen.label_moments(tx, pb, M, 0, 64, L.DPI_BOTH, ws),
                         gen.label_moments(tx, pb, M, 64, M, L.DPI_BOTH, ws)]).contiguous()
    red = gen.moments_reduce(parts)
    assert torch.isfinite(full).all() and torch.equal(red, full)


def test_stash_reuse():
    """4 points x 1,024 blocks = 4,096 blocks on a fixed number of stash slots (several launches of block
    ranges), more than 64 blocks per point (the k_reduce launch, not the fused reduce): point 0 against
    the oracle, and the whole call bit-identical to four one-point calls."""
    n, M_ = 4, 65536
    eq, oeq = T.equation("ou", 7)
    inner = T.scaled_mlp("ou", V, "ELU", [24] * 5, 7, scales=(2.0, 256.0))  # gates (a), (b) at point 0: see _gated_ref
    module, twin = PicardSolutionEnforceTerminal(eq, inner, V), T.from_module(oeq, inner, ["ELU"] * 5, V)
    gen = _gen(eq, module, M_=M_, K_=1)
    _is_terminal(gen, V)
    slots = gen.net.general_slots()
    assert n * (M_ // 64) > 2 * slots
    tx, pb = gen.sample_t_and_x(n, point_base=0)
    y = gen.generate_with_gradients(tx, point_base=pb)
    ref = _gated_ref(oeq, twin, tx[:1].cpu().double().numpy(), M_, 1)
    _check(y[:1].cpu().numpy(), ref, "stash reuse, point 0")
    for i in range(n):
        yi = gen.generate_with_gradients(tx[i:i + 1].contiguous(), point_base=pb + i)
        assert torch.equal(yi, y[i:i + 1]), i


@pytest.mark.parametrize("kind", [V, OG])
def test_workspace_counts_the_stash(kind):
    """The Value form parks act' as every general value net does, [128] * 4 included; the OnlyGradient
    form has no stash."""
    nx, n = 100, 16
    eq, _ = T.equation("cha", nx)
    g_term = _gen(eq, PicardSolutionEnforceTerminal(eq, T.scaled_mlp("cha", kind, "ELU", [128] * 4, nx), kind))
    g_spec = _gen(eq, T.scaled_mlp("cha", V, "ELU", [128] * 4, nx))  # the plain net: specialised, no stash
    assert _family(g_spec) == L.DPI_FAMILY_SPECIALISED and g_spec.net.general_slots() == 0
    a, b = g_term.workspace_bytes(n, M), g_spec.workspace_bytes(n, M)
    if kind == V:
        assert g_term.net.general_slots() == 512 and a - b >= 512 * 3 * 8 * 256 * 16
    else:
        assert g_term.net.general_slots() == 0 and a < b + 512 * 3 * 8 * 256 * 16


@pytest.mark.parametrize("kind,nx", [(V, 7), (OG, 127)])
def test_canary(kind, nx):
    """[256] * 8, M = 100 (a partial block), nx no multiple of the tile: nothing is written past the
    workspace (the Value form's last region is the stash), the moments or the labels (the pattern of
    tests/test_gpu_canary.py)."""
    from test_gpu_canary import Carved, _stream
    n, M_ = 3, 100
    eq, _ = T.equation("ou", nx)
    module = PicardSolutionEnforceTerminal(eq, T.scaled_mlp("ou", kind, "ELU", [256] * 8, nx), kind)
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


# ------------------------------------------------------------------------------- refusals
def _gbm(nx):
    rng = np.random.default_rng(nx)
    w = rng.standard_normal((2, 1 + nx)) / np.sqrt(nx)
    w[:, 0] = 1.0
    return dpi.GBMEquationComplexExact(nx, 1.0, 1.0, w=w, v=rng.standard_normal((2, 1)))


@pytest.mark.parametrize("kind", [V, OG])
@pytest.mark.parametrize("what", ["gbm", "td", "nx129"])
def test_refusals_name_their_cap(what, kind):
    nx = 129 if what == "nx129" else 7
    eq = _gbm(nx) if what == "gbm" else T.equation("cha", nx)[0]
    module = PicardSolutionEnforceTerminal(eq, T.scaled_mlp("cha", kind, "ELU", [40], nx), kind)
    gen = _gen(eq, module, estimate_delta_t=0.3 if what == "td" else None)
    word = {"gbm": "GBM", "td": "TD", "nx129": "128"}[what]
    with pytest.raises(DPIError, match=word) as ei:
        gen.generate_with_gradients(*gen.sample_t_and_x(N, point_base=0))
    assert f"({L.DPI_ERR_UNSUPPORTED})" in str(ei.value) and "terminal-enforcing" in str(ei.value)
    with pytest.raises(DPIError, match=word):
        _family(gen, td=what == "td")


@pytest.mark.parametrize("kind", [V, OG])
def test_hessian_labels_are_refused(kind):
    eq, _ = T.equation("cha", 7)
    gen = _gen(eq, PicardSolutionEnforceTerminal(eq, T.scaled_mlp("cha", kind, "ELU", [40], 7), kind))
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    with pytest.raises(DPIError, match="Hessian") as ei:
        gen.generate_with_gradients_and_hessians(tx, point_base=pb)
    assert f"({L.DPI_ERR_UNSUPPORTED})" in str(ei.value) and "terminal-enforcing" in str(ei.value)
    assert _family(gen) == L.DPI_FAMILY_GENERAL  # the first-order labels of the pair run


def test_equation_mismatch_is_refused():
    """The wrapper's equation against the generator's, by value; and the net's T against the problem's
    at the label call (DPI_ERR_ARG)."""
    nx = 7
    inner = T.scaled_mlp("cha", V, "ELU", [40], nx)
    w = PicardSolutionEnforceTerminal(dpi.Cha(nx, 1.0, 5.0, 2.0), inner, V)
    with pytest.raises(ValueError, match="T=2.0"):
        _gen(dpi.Cha(nx, 1.0, 5.0, 1.0), w)
    gen = _gen(dpi.Cha(nx, 1.0, 5.0, 2.0), w)  # another object with equal values: accepted
    other = _gen(dpi.Cha(nx, 1.0, 5.0, 1.0), T.scaled_mlp("cha", V, "ELU", [40], nx))
    tx, pb = other.sample_t_and_x(N, point_base=0)
    other.net = gen.net  # a net built for T = 2 on a problem with T = 1
    with pytest.raises(DPIError, match="another T") as ei:
        other.generate_with_gradients(tx, point_base=pb)
    assert f"({L.DPI_ERR_ARG})" in str(ei.value)


# ------------------------------------------------------------------------------- the silent failure
@pytest.mark.parametrize("eq_kind,kind", [("cha", V), ("ou", V), ("cha", OG), ("ou", OG)])
def test_the_wrapper_is_not_uploaded_as_its_bare_model(eq_kind, kind):
    """The same module labelled through DeviceNet.from_module: its labels match the oracle's ansatz labels
    and differ from its bare .model's by >= 1e-2 — also inside a gradient wrapper's `.solution`."""
    eq, oeq, module, twin = _case(eq_kind, kind, "Tanh", "w64x4", 7)

    class GradientWrapper(torch.nn.Module):  # PicardSolutionGradientWrapper's shape (solution_jac.py:124-126)
        def __init__(self, solution):
            super().__init__()
            self.solution = solution

    gen = _gen(eq, GradientWrapper(module))
    _is_terminal(gen, kind)
    bare = _gen(eq, module.model)
    assert not bare.net.desc.endswith("-terminal")
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    ref = _gated_ref(oeq, twin, tx.cpu().double().numpy())
    y = gen.generate_with_gradients(tx, point_base=pb).cpu().numpy()
    yb = bare.generate_with_gradients(tx, point_base=pb).cpu().numpy()
    _check(y, ref, (eq_kind, kind, "wrapper"))
    d = O.rel_l2_parts(yb, y)
    assert d["value"] >= 1e-2 and d["grad"] >= 1e-2, d


# ------------------------------------------------------------------------------- picard train
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
  SEED: 3
  kwargs: {{t_always_uniform: true, n_estimate_terminal: 256, n_estimate_integral: 256}}
TRAIN:
  N_EPOCHS: 4
  BATCH_SIZE: 128
  SUPERVISE_GRADIENT: true
  LOSS: {{beta: 0.0, SCALER: {{cls: FixedLossScaler, kwargs: {{fixed_weight: 0.1}}}}}}
  OPTIMIZER: {{kwargs: {{lr: 0.003}}}}
NETWORK:
  cls: PicardSolutionEnforceTerminal
  TYPE: {typ}
  NEURONS: [24, 24, 24]
  ACTIVATIONS: [Tanh, Tanh, Tanh]
  BOUND: None
  RELOAD: true
EVAL: {{L2_N_POINTS: 256}}
"""


@pytest.mark.parametrize("typ", [V, OG])
def test_picard_train_with_a_terminal_enforcing_net(tmp_path, typ):
    """`picard train` with NETWORK.cls PicardSolutionEnforceTerminal: iteration 1 starts from ZeroSolution,
    iteration 2's labels come from the fitted wrapper — its first two points against the oracle on the
    fitted weights — and the checkpoint holds the wrapper's state."""
    from deeppicarditeration_amd.config import load_cfg
    from deeppicarditeration_amd.runner import PicardRunner
    f = tmp_path / "term.yaml"
    f.write_text(TRAIN.format(name=tmp_path / "run", typ=typ))
    runner = PicardRunner(load_cfg(str(f)))
    seen = {}
    orig = runner.labels

    def labels():
        u = runner.u_current
        seen[runner.i] = (type(u).__name__, {k: v.detach().cpu().clone() for k, v in u.state_dict().items()}, *orig())
        return seen[runner.i][2:]

    runner.labels = labels
    hist = runner.run()
    assert [h["iter"] for h in hist] == [1, 2] and all(h["labels"] == 512 for h in hist)
    assert seen[1][0] == "ZeroSolution" and seen[2][0] == "PicardSolutionEnforceTerminal"
    _, sd1, tx, y = seen[2]
    assert torch.isfinite(y).all() and y.shape == (512, 9)
    idx = sorted({int(k.split(".")[1]) for k in sd1 if k.startswith("model.")})
    oeq = O.Cha(8, 1.0, 5.0, 1.0)
    twin = T.TerminalNet(oeq, T.inner_net([sd1[f"model.{i}.weight"].double().numpy() for i in idx],
                                          [sd1[f"model.{i}.bias"].double().numpy() for i in idx], ["Tanh"] * 3, typ), typ)
    ref = O.labels_grad(oeq, twin, tx[:2].cpu().double().numpy(), 256, 4, 3, 2, 0)
    _check(y[:2].cpu().double().numpy(), ref, ("picard train", typ, "iteration-2 labels"))
    sd = torch.load(tmp_path / "run" / "model_2.pt", weights_only=True)
    assert "T" in sd and list(sd.values())[-1].shape == ((1,) if typ == V else (8,))
    recs = [json.loads(l) for l in (tmp_path / "run" / "history.jsonl").read_text().splitlines()]
    assert len(recs) == 2
    for r in recs:
        assert r["fit"] == ("gradient" if typ == V else "head_only_gradient")
        assert r["labels_per_s"] > 0 and np.isfinite(r["loss"]) and np.isfinite(r["rel_l2_u"])


def test_gbm_is_the_label_calls_error(tmp_path):
    """NETWORK.cls PicardSolutionEnforceTerminal on GBM: the runner builds the wrapper, and the label
    call of the iteration that starts from it refuses the pair by name."""
    from deeppicarditeration_amd.config import load_cfg
    from deeppicarditeration_amd.runner import PicardRunner
    f = tmp_path / "gbm.yaml"
    text = TRAIN.format(name=tmp_path / "run", typ=V).replace("cls: Cha", "cls: GBMEquationComplexExact").replace(
        "{nx: 8, alpha: 1.0, k: 5.0, T: 1.0}", "{nx: 100, alpha: 1.0, T: 1.0}").replace("DATA_SIZE: 512", "DATA_SIZE: 256")
    f.write_text(text)
    runner = PicardRunner(load_cfg(str(f)))
    runner.i, runner.u_current = 1, runner.new_network()
    with pytest.raises(DPIError, match="GBM") as ei:
        runner.labels()
    assert "terminal-enforcing" in str(ei.value)


NEST = """NAME: {name}
EQUATION:
  cls: OUProcessEquation
  kwargs: {{nx: 10, alpha: 1.0, T: 1.0, num_components: 5, mean_scale: 1.0, var_scale: 2.0, alpha_scale: 4.0,
           mean: {mean}, pi: {pi}}}
METHOD:
  cls: DeepNesting
PICARD: {{N: 2}}
FORCE: true
DATA:
  FLOAT: float
  DATA_SIZE: 256
  POINTS_PER_CALL: 128
  kwargs: {{t_always_uniform: true, n_estimate_terminal: 256, n_estimate_integral: 256}}
TRAIN:
  N_EPOCHS: 2
  BATCH_SIZE: 64
  SUPERVISE_GRADIENT: true
  LOSS: {{beta: 0.0, SCALER: {{cls: FixedLossScaler, kwargs: {{fixed_weight: 1.0}}}}}}
  OPTIMIZER: {{kwargs: {{lr: 0.001}}}}
NETWORK:
  cls: PicardSolution
  NEURONS: [64, 64, 64, 64]
  ACTIVATIONS: ["ELU", "ELU", "ELU", "ELU"]
  BOUND: None
  RELOAD: true
  PISGRADNET: true
EVAL: {{L2_N_POINTS: 100, TEST_GRAD: true}}
"""


def test_picard_train_deep_nesting_yaml(tmp_path):
    """scripts/hjb/hjb_nest_10d_T1.0_w1.0.yaml's keys scaled down (METHOD.cls DeepNesting, OU nx = 10,
    PISGradNet [64] * 4): the reference sends it down the Picard path (picard_iteration.py:253-264), and
    so does the runner; it runs to the end.  The mixture's parameters are given inline (the reference
    draws them at nx != 100)."""
    from deeppicarditeration_amd.config import load_cfg
    from deeppicarditeration_amd.runner import PicardRunner
    rng = np.random.default_rng(10)
    mean, pi = rng.uniform(-1, 1, (5, 10)).round(4), rng.uniform(0.1, 1, 5)
    f = tmp_path / "nest.yaml"
    f.write_text(NEST.format(name=tmp_path / "run", mean=json.dumps(mean.tolist()),
                             pi=json.dumps((pi / pi.sum()).tolist())))
    hist = PicardRunner(load_cfg(str(f))).run()
    assert [h["iter"] for h in hist] == [1, 2]
    assert all(np.isfinite(h["loss"]) and h["rel_l2_u"] is not None for h in hist)
    assert (tmp_path / "run" / "model_2.pt").exists()
