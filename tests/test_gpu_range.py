"""Range and precision of the fp16-split MFMA default under large weights,
with the fp64 oracle as the judge (VERDICT r2 "weak" 2): every network parameter multiplied by s
(tests/golden/make_golden.py's weight_scale), both GEMM modes, and the range guard
(include/dpi.h dpi_net_status) where the split storage overflows.

Measured bound (tools/probe_range.py, profiles/r03b_probe_range.jsonl): the fused MLPs stay within
rel-L2 1e-4 of the oracle for s <= 32 (Cha 4 x 128: labels up to 2e10) in both modes; GBM 3 x 64's
SDGD labels lose accuracy past s = 16 in BOTH modes (fp32's own conditioning of f = ... |u_ii| terms at
labels ~1e5, not the split); the PISGradNet split storage overflows fp16 past s ~ 12 (labels ~1e21),
where the guard recomputes in fp32."""
import warnings

import numpy as np
import pytest
import torch

from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(params=["auto", "f32"])
def mode(request):
    from deeppicarditeration_amd import _lib as L
    L.check(L.load().dpi_set_gemm_precision(L.DPI_GEMM_AUTO if request.param == "auto" else L.DPI_GEMM_F32), "prec")
    yield request.param
    L.check(L.load().dpi_set_gemm_precision(L.DPI_GEMM_AUTO), "prec")


def _scaled(net, s):
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(s)
    return net


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _mlp_oracle(net):
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    return O.MLP([m.weight.detach().double().numpy() for m in lin], [m.bias.detach().double().numpy() for m in lin],
                 ["ELU"] * (len(lin) - 1))


@pytest.mark.parametrize("eqname, widths, scale", [("cha", [128] * 4, 8.0), ("cha", [128] * 4, 32.0),
                                                   ("cha", [128] * 4, 1 / 32), ("gbm", [64] * 3, 8.0),
                                                   ("gbm", [64] * 3, 16.0)])
def test_scaled_mlp_vs_oracle(mode, eqname, widths, scale):
    import deeppicarditeration_amd as dpi
    torch.manual_seed(3)
    if eqname == "cha":
        eq, oeq, v = dpi.Cha(100, 1.0, 5.0, 1.0), O.Cha(100, 1.0, 5.0, 1.0), 0
    else:
        eq = dpi.GBMEquationComplexExact(100)
        oeq, v = O.GBMEquationComplexExact(100, eq.w.numpy(), eq.v.numpy()), 100
    net = _scaled(dpi.construct_mlp(101, 1, widths, ["ELU"] * len(widths), None), scale)
    gen = dpi.OnlineDataGenerator(eq, net, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=256,
                                  n_estimate_integral=256, n_euler_steps=10, seed=1,
                                  hessian_approximation={"method": "SDGD", "kwargs": {"v": v}} if v else None)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no fallback needed: the fused MLP stays in range
        tx, y = gen.sample_with_gradients(2)
    ref = O.labels_grad(oeq, _mlp_oracle(net), tx.cpu().double().numpy(), 256, 10, 1, 1, 0, v=v)
    y = y.cpu().double().numpy()
    ev, eg = _rel(y[:, :1], ref[:, :1]), _rel(y[:, 1:], ref[:, 1:])
    print(f"{eqname} x{scale} {mode}: max|label| {np.abs(ref).max():.2e} value {ev:.2e} grad {eg:.2e}")
    assert ev < TOL and eg < TOL


def _pis(scale):
    import deeppicarditeration_amd as dpi
    eq = dpi.OUProcessEquation(nx=100, T=1.0, alpha=1.0, num_components=5, mean_scale=1.0, var_scale=2.0,
                               alpha_scale=4.0)
    torch.manual_seed(7)
    net = _scaled(dpi.PISGradNet(hidden_shapes=[512] * 4, dim=100, g0=eq.g, T=1.0), scale)
    with torch.no_grad():
        net.timestep_phase.copy_(0.1 * torch.randn(1, 64))
    gen = dpi.OnlineDataGenerator(eq, net, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=128,
                                  n_estimate_integral=128, n_euler_steps=10, seed=2)
    oeq = O.OUProcessEquation(100, eq.mean.numpy(), eq.var.numpy(), eq.pi.numpy(), alpha_scale=4.0)
    onet = O.PISGradNet({k: v.detach().double().numpy() for k, v in net.state_dict().items()}, oeq, T=1.0)
    return gen, oeq, onet


@pytest.mark.parametrize("scale", [8.0, 32.0])
def test_scaled_pisgradnet_vs_oracle(mode, scale):
    """PISGradNet 4 x 512: at 8x both modes match the oracle directly; at 32x the split storage
    overflows fp16 (labels ~1e29) and the range guard recomputes the call in exact fp32 with a
    SplitRangeWarning — never a silent inf / NaN label."""
    from deeppicarditeration_amd.data import SplitRangeWarning
    gen, oeq, onet = _pis(scale)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tx, y = gen.sample_with_gradients(2)
    fell_back = any(issubclass(x.category, SplitRangeWarning) for x in w)
    assert fell_back == (mode == "auto" and scale == 32.0), [str(x.message) for x in w]
    assert bool(torch.isfinite(y).all())
    ref = O.labels_grad(oeq, onet, tx.cpu().double().numpy(), 128, 10, 2, 1, 0)
    y = y.cpu().double().numpy()
    ev, eg = _rel(y[:, :1], ref[:, :1]), _rel(y[:, 1:], ref[:, 1:])
    print(f"pis x{scale} {mode}: max|label| {np.abs(ref).max():.2e} value {ev:.2e} grad {eg:.2e} fallback {fell_back}")
    assert ev < TOL and eg < TOL
    if fell_back:  # the generator stays in fp32: no further flag, no further warning
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _, y2 = gen.sample_with_gradients(2)
        assert bool(torch.isfinite(y2).all()) and gen.range_status() == 0


def test_fp32_overflow_raises():
    """Labels beyond fp32's range from finite weights: a loud DPIError (after the fp32 retry)."""
    import deeppicarditeration_amd as dpi
    from deeppicarditeration_amd._lib import DPIError
    eq = dpi.Cha(100, 1.0, 5.0, 1.0)
    torch.manual_seed(3)
    net = _scaled(dpi.construct_mlp(101, 1, [32, 32], ["ELU"] * 2, None), 1e13)
    gen = dpi.OnlineDataGenerator(eq, net, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=64,
                                  n_estimate_integral=64, n_euler_steps=2, seed=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(DPIError, match="fp32"):
            gen.sample_with_gradients(2)


def test_nan_parameters_are_not_flagged():
    """NaN weights give NaN labels as in the reference (torch propagates them): no flag, no error."""
    import deeppicarditeration_amd as dpi
    eq = dpi.Cha(100, 1.0, 5.0, 1.0)
    torch.manual_seed(0)
    net = dpi.construct_mlp(101, 1, [32, 32], ["ELU", "ELU"], None)
    with torch.no_grad():
        net[0].weight[0, 0] = float("nan")
    gen = dpi.OnlineDataGenerator(eq, net, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=64,
                                  n_estimate_integral=64, n_euler_steps=2, seed=1)
    _, y = gen.sample_with_gradients(2)
    assert bool(torch.isnan(y).any()) and gen.range_status() == 0


@pytest.mark.parametrize("case", ["cha_mlp128x4_ws8_K3", "cha_mlp128x4_ws32_K3", "ou_pis32_ws8_K2", "ou_pis32_ws32_K2"])
def test_weight_scaled_goldens_both_modes(mode, case):
    """The reference's own labels for networks with every parameter scaled by 8 and 32
    (tests/golden/make_golden.py weight_scale), in both GEMM modes: rel-L2 <= 1e-4, through the
    range guard where the split storage leaves fp16's range."""
    from golden_util import load
    from gpu_util import generator, product_equation, product_module, rel_l2_parts
    f = load(case)
    eq = product_equation(f)
    gen = generator(f, eq, product_module(f, eq))
    tx = torch.as_tensor(f["tx"], dtype=torch.float32, device="cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = gen.generate_with_gradients(tx, point_base=int(f["point_base"])).cpu().numpy()
    parts = rel_l2_parts(y, f["y"])
    print(case, mode, f"max|y| {np.abs(f['y']).max():.2e}", parts, "fp32 fallback:", gen._fp32_fallback)
    assert parts["value"] < TOL and parts["grad"] < TOL, parts


# ---------------------------------------------------------------- the deferred guard (RangeGroup)
def _fp32_twin(scale):
    """The same generator state forced to exact fp32: what a repaired call must equal bit for bit."""
    gen, _, _ = _pis(scale)
    gen.use_fp32()
    return gen


def test_range_group_repairs_its_calls_in_place():
    """Split-mode PISGradNet at 32x (fp16 overflow) inside deferred_range_check(): no stream
    synchronisation per call, the non-finite labels sit in the returned tensors until verify(),
    which warns, switches the net to fp32 and rewrites those tensors — equal to fp32 calls on the
    same counters and within 1e-4 of the oracle."""
    from deeppicarditeration_amd.data import SplitRangeWarning
    gen, oeq, onet = _pis(32.0)
    with gen.deferred_range_check() as grp:
        tx1, y1 = gen.sample_with_gradients(2)
        tx2, y2 = gen.sample_with_gradients(3)
    with pytest.warns(SplitRangeWarning):
        flag = grp.verify()
    assert flag == 1 and gen._fp32_fallback
    ref = _fp32_twin(32.0)
    for tx, y in ((tx1, y1), (tx2, y2)):
        txr, yr = ref.sample_with_gradients(tx.shape[0])
        assert torch.equal(tx, txr) and torch.equal(y, yr)
    o = O.labels_grad(oeq, onet, tx1.cpu().double().numpy(), 128, 10, 2, 1, 0)
    y = y1.cpu().double().numpy()
    assert _rel(y[:, :1], o[:, :1]) < TOL and _rel(y[:, 1:], o[:, 1:]) < TOL


def test_range_group_without_overflow_changes_nothing():
    """A group whose calls stay in range verifies to 0: no warning, labels bitwise the per-call
    guarded ones, the net stays on the split MFMA."""
    a, _, _ = _pis(1.0)
    b, _, _ = _pis(1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with a.deferred_range_check() as grp:
            ya = [a.sample_with_gradients(2)[1] for _ in range(3)]
        assert grp.verify() == 0
    yb = [b.sample_with_gradients(2)[1] for _ in range(3)]
    assert all(torch.equal(p, q) for p, q in zip(ya, yb)) and not a._fp32_fallback


def test_dataset_surface_verifies_each_buffer_before_yielding_it():
    """dataset_with_gradients (the boundary the reference's data module pulls from): every yielded
    batch is finite and equals the fp32 labels, with one SplitRangeWarning, at no per-call sync."""
    from deeppicarditeration_amd.data import SplitRangeWarning
    gen, _, _ = _pis(32.0)
    ds = gen.dataset_with_gradients(12, 1, 4)  # 3 buffers of one 4-point call each
    with pytest.warns(SplitRangeWarning):
        batches = list(ds)
    ref = _fp32_twin(32.0)
    for x, y in batches:
        xr, yr = ref.sample_with_gradients(4)
        assert torch.equal(x, xr) and torch.equal(y, yr)
        assert torch.isfinite(y).all()


def test_label_buffer_fill_is_one_range_group():
    """picard train's LabelBuffer.fill: its calls form one group, checked once after the fill."""
    from deeppicarditeration_amd.data import SplitRangeWarning
    from deeppicarditeration_amd.runner import LabelBuffer
    gen, _, _ = _pis(32.0)
    with pytest.warns(SplitRangeWarning):
        tx, y = LabelBuffer(gen.sample_with_gradients, 6, 2, guard=gen).fill()
    ref = _fp32_twin(32.0)
    txr, yr = LabelBuffer(ref.sample_with_gradients, 6, 2, guard=ref).fill()
    assert torch.equal(tx, txr) and torch.equal(y, yr)


def test_pipeline_flag_survives_a_later_begin():
    """a flagged begin/end batch followed by another begin/end must still be caught by
    pipeline_range_check() (begin() no longer clears the status; each pipeline has its own slot),
    which repairs both batches' labels in place."""
    from deeppicarditeration_amd.data import SplitRangeWarning
    from deeppicarditeration_amd.sharding import ShardedLabeler
    gen, _, _ = _pis(32.0)
    lab = ShardedLabeler(gen)
    out = []
    for _ in range(2):
        tx, pb = gen.sample_t_and_x(2)
        out.append((tx, pb, lab.end(lab.begin(tx, pb))))
    with pytest.warns(SplitRangeWarning):
        assert lab.pipeline_range_check() == 1
    for tx, pb, y in out:
        assert torch.isfinite(y).all()
        assert torch.equal(y, ShardedLabeler(gen).labels(tx, pb))  # the net is fp32 now


def test_range_group_fp32_overflow_raises():
    """Labels beyond fp32's range inside a group: verify() raises DPIError after the fp32 retry."""
    import deeppicarditeration_amd as dpi
    from deeppicarditeration_amd._lib import DPIError
    eq = dpi.Cha(100, 1.0, 5.0, 1.0)
    torch.manual_seed(3)
    net = _scaled(dpi.construct_mlp(101, 1, [32, 32], ["ELU"] * 2, None), 1e13)
    gen = dpi.OnlineDataGenerator(eq, net, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=64,
                                  n_estimate_integral=64, n_euler_steps=2, seed=1)
    with gen.deferred_range_check() as grp:
        gen.sample_with_gradients(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(DPIError, match="fp32"):
            grp.verify()


# ------------------------------------------------- small magnitudes
# Networks scaled DOWN: every parameter x 1/16 and x 1/256 ("wsd"), and rescaled so every hidden
# activation is ~1/256 as large while the function stays about the same ("homog": first layer x s,
# the other hidden biases x s, output weights x 1/s).  The split storage keeps each operand at a
# calibrated power-of-two scale (dpi_net_image.h x3_exponent), so its labels must stay fp32-class:
# within 10x of the exact-fp32 mode's rel-L2 on the same inputs (or 2e-7, the labels' own fp32
# rounding, whichever is larger), and within the 1e-4 bar.
SMALL = ["ou_pis32_wsd16_K2", "ou_pis32_wsd256_K2", "ou_pis32_homog256_K2", "gbm_mlp16_sdgd_wsd16_K2",
         "gbm_mlp16_sdgd_wsd256_K2", "gbm_mlp64x3_sdgd_wsd16_K2", "gbm_mlp64x3_sdgd_wsd256_K2",
         "gbm_mlp64x3_sdgd_homog256_K2", "cha_mlp128x4_homog256_K3"]
SMALL_HESS = ["gbm_hess_mlp32x3_wsd16_K2", "gbm_hess_mlp32x3_wsd256_K2", "gbm_hess_mlp32x3_homog256_K2"]
FP32_CLASS = 10.0
FLOOR = 2e-7


def _both_modes(label):
    """label() -> labels, evaluated in split (auto) then exact-fp32 mode."""
    from deeppicarditeration_amd import _lib as L
    lib = L.load()
    out = {}
    try:
        for name, mode in (("auto", L.DPI_GEMM_AUTO), ("f32", L.DPI_GEMM_F32)):
            L.check(lib.dpi_set_gemm_precision(mode), "prec")
            with warnings.catch_warnings():
                warnings.simplefilter("error")  # no range fallback: the split itself must hold
                out[name] = label()
    finally:
        L.check(lib.dpi_set_gemm_precision(L.DPI_GEMM_AUTO), "prec")
    return out


def _assert_fp32_class(errs, blocks):
    for b in blocks:
        a, f = errs["auto"][b], errs["f32"][b]
        assert a < TOL and a <= max(FP32_CLASS * f, FLOOR), (b, errs)


@pytest.mark.parametrize("case", SMALL + SMALL_HESS)
def test_down_scaled_goldens_split_is_fp32_class(case):
    from golden_util import load
    from gpu_util import generator, product_equation, product_module
    f = load(case)
    eq = product_equation(f)
    tx = torch.as_tensor(f["tx"], dtype=torch.float32, device="cuda:0")
    hess = case in SMALL_HESS

    def label():
        gen = generator(f, eq, product_module(f, eq))
        if hess:
            return gen.generate_with_gradients_and_hessians(tx, point_base=int(f["point_base"])).cpu().numpy()
        return gen.generate_with_gradients(tx, point_base=int(f["point_base"])).cpu().numpy()

    ys = _both_modes(label)
    blocks = {"value": slice(0, 1), "grad": slice(1, 101), "hess": slice(101, None)}
    errs = {m: {b: _rel(y[:, sl], f["y"][:, sl]) for b, sl in blocks.items() if hess or b != "hess"}
            for m, y in ys.items()}
    print(case, errs)
    _assert_fp32_class(errs, errs["auto"].keys())


def _scale_down(lin, s, how):
    with torch.no_grad():
        if how == "all":
            for m in lin:
                m.weight.mul_(s)
                m.bias.mul_(s)
        else:  # homog
            lin[0].weight.mul_(s)
            for m in lin[:-1]:
                m.bias.mul_(s)
            lin[-1].weight.mul_(1.0 / s)


@pytest.mark.parametrize("s, how", [(1 / 16, "all"), (1 / 256, "all"), (1 / 256, "homog"), (1 / 4096, "homog")])
def test_down_scaled_pisgradnet_4x512_vs_oracle(s, how):
    """PISGradNet 4 x 512 (configs[2]'s network, the fused k_pis_net chain) scaled down, both modes,
    against the fp64 oracle."""
    import deeppicarditeration_amd as dpi
    eq = dpi.OUProcessEquation(nx=100, T=1.0, alpha=1.0, num_components=5, mean_scale=1.0, var_scale=2.0,
                               alpha_scale=4.0)
    torch.manual_seed(7)
    net = dpi.PISGradNet(hidden_shapes=[512] * 4, dim=100, g0=eq.g, T=1.0)
    with torch.no_grad():
        net.timestep_phase.copy_(0.1 * torch.randn(1, 64))
    _scale_down([m for m in net.nn_module if isinstance(m, torch.nn.Linear)], s, how)
    oeq = O.OUProcessEquation(100, eq.mean.numpy(), eq.var.numpy(), eq.pi.numpy(), alpha_scale=4.0)
    onet = O.PISGradNet({k: v.detach().double().numpy() for k, v in net.state_dict().items()}, oeq, T=1.0)
    tx = None

    def label():
        nonlocal tx
        gen = dpi.OnlineDataGenerator(eq, net, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=128,
                                      n_estimate_integral=128, n_euler_steps=10, seed=2)
        tx, y = gen.sample_with_gradients(2)
        return y.cpu().double().numpy()

    ys = _both_modes(label)
    ref = O.labels_grad(oeq, onet, tx.cpu().double().numpy(), 128, 10, 2, 1, 0)
    errs = {m: {"value": _rel(y[:, :1], ref[:, :1]), "grad": _rel(y[:, 1:], ref[:, 1:])} for m, y in ys.items()}
    print(f"pis x{s} {how}", errs)
    _assert_fp32_class(errs, ("value", "grad"))


@pytest.mark.parametrize("s, how", [(1 / 16, "all"), (1 / 256, "all"), (1 / 256, "homog"), (1 / 4096, "homog")])
@pytest.mark.parametrize("hess", [False, True])
def test_down_scaled_gbm_3x64_vs_oracle(s, how, hess):
    """GBM 3 x 64 (configs[4]'s network: the split SDGD tangent sweep, and the Malliavin Hessian
    labels' three sweeps) scaled down, both modes, against the fp64 oracle."""
    import deeppicarditeration_amd as dpi
    eq = dpi.GBMEquationComplexExact(100)
    oeq = O.GBMEquationComplexExact(100, eq.w.numpy(), eq.v.numpy())
    torch.manual_seed(3)
    net = dpi.construct_mlp(101, 1, [64] * 3, ["ELU"] * 3, None)
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    _scale_down(lin, s, how)
    onet = O.MLP([m.weight.detach().double().numpy() for m in lin], [m.bias.detach().double().numpy() for m in lin],
                 ["ELU"] * 3)
    tx = None

    def label():
        nonlocal tx
        gen = dpi.OnlineDataGenerator(eq, net, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=256,
                                      n_estimate_integral=256, n_euler_steps=10, seed=1,
                                      hessian_approximation=None if hess else {"method": "SDGD", "kwargs": {"v": 100}})
        tx, y = gen.sample_with_gradients_and_hessians(2) if hess else gen.sample_with_gradients(2)
        return y.cpu().double().numpy()

    ys = _both_modes(label)
    txh = tx.cpu().double().numpy()
    ref = O.labels_grad_hess(oeq, onet, txh, 256, 10, 1, 1, 0) if hess else O.labels_grad(oeq, onet, txh, 256, 10, 1,
                                                                                         1, 0, v=100)
    blocks = {"value": slice(0, 1), "grad": slice(1, 101), "hess": slice(101, None)}
    errs = {m: {b: _rel(y[:, sl], ref[:, sl]) for b, sl in blocks.items() if hess or b != "hess"} for m, y in ys.items()}
    print(f"gbm x{s} {how} hess={hess}", errs)
    _assert_fp32_class(errs, errs["auto"].keys())
