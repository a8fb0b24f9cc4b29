"""TRAIN.FUSED_STEP and the step it selects (config.py, fit.build_objective, fit.device_step) — CPU only.  Off,
the default, builds what was built before the key existed; on, under TRAIN.BACKEND: hip, it builds the
device step, and everything the fused step does not cover is refused by name — at configuration load where
the configuration shows it, otherwise at the first batch before the library is touched — never falling
back."""
import pytest
import torch

from deeppicarditeration_amd import fit
from deeppicarditeration_amd.config import get_default_cfg, load_cfg
from deeppicarditeration_amd.solution import PISGradNet, construct_mlp


def _yaml(tmp_path, train="", network=""):
    f = tmp_path / "a.yaml"
    f.write_text(f"NAME: x\nTRAIN: {{{train}}}\nNETWORK: {{{network}}}\n")
    return str(f)


def test_key_defaults_to_false_and_loads(tmp_path):
    assert get_default_cfg().TRAIN.FUSED_STEP is False
    assert load_cfg(_yaml(tmp_path)).TRAIN.FUSED_STEP is False
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip, FUSED_STEP: true")).TRAIN.FUSED_STEP is True
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip"), ["TRAIN.FUSED_STEP", "True"]).TRAIN.FUSED_STEP is True
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip, FUSED_STEP: true"),
                    ["TRAIN.FUSED_STEP", "False"]).TRAIN.FUSED_STEP is False
    cfg = load_cfg(_yaml(tmp_path, "BACKEND: hip, FUSED_STEP: true, OPTIMIZER: {cls: AdamW, kwargs: {lr: 0.01}}"))
    assert cfg.TRAIN.OPTIMIZER.cls == "AdamW"
    with pytest.raises(ValueError, match="TRAIN.FUSED_STEP"):
        load_cfg(_yaml(tmp_path, "BACKEND: hip, FUSED_STEP: maybe"))


@pytest.mark.parametrize("train, network, named", [
    ("FUSED_STEP: true", "", "TRAIN.BACKEND: torch"),
    ("BACKEND: hip, FUSED_STEP: true, OPTIMIZER: {cls: SGD, kwargs: {lr: 0.1}}", "", "TRAIN.OPTIMIZER.cls SGD"),
    ("BACKEND: hip, FUSED_STEP: true, OPTIMIZER: {kwargs: {amsgrad: true}}", "", "amsgrad"),
    ("BACKEND: hip, FUSED_STEP: true, OPTIMIZER: {kwargs: {maximize: true}}", "", "maximize"),
    ("BACKEND: hip, FUSED_STEP: true, OPTIMIZER: {kwargs: {capturable: true}}", "", "capturable"),
    ("BACKEND: hip, FUSED_STEP: true, OPTIMIZER: {kwargs: {differentiable: true}}", "", "differentiable"),
    ("BACKEND: hip, FUSED_STEP: true", "PISGRADNET: true", "NETWORK.PISGRADNET"),
], ids=["torch_backend", "sgd", "amsgrad", "maximize", "capturable", "differentiable", "pisgradnet"])
def test_configuration_refusals_at_load(tmp_path, train, network, named):
    with pytest.raises(NotImplementedError, match=named) as e:
        load_cfg(_yaml(tmp_path, train, network))
    assert "TRAIN.FUSED_STEP" in str(e.value)


def test_build_objective_selects_the_step():
    t = get_default_cfg().TRAIN
    for sg, want in ((False, "value"), (True, "gradient")):
        step, kind = fit.build_objective(t, 4, sg, False, backend="hip", fused_step=True)
        assert kind == want and step.__qualname__.startswith("device_step.")
        obj, kind = fit.build_objective(t, 4, sg, False, backend="hip")
        assert kind == want and obj.__qualname__.startswith("device_objective.")
    with pytest.raises(NotImplementedError, match="TRAIN.BACKEND: torch") as e:
        fit.build_objective(t, 4, True, False, backend="torch", fused_step=True)
    assert "TRAIN.FUSED_STEP" in str(e.value)
    # what TRAIN.BACKEND: hip refuses stays refused, with its text
    t.LOSS.SCALER = {"cls": "SimpleLossScaler", "kwargs": {}}
    with pytest.raises(NotImplementedError, match="TRAIN.BACKEND: hip with TRAIN.LOSS.SCALER SimpleLossScaler"):
        fit.build_objective(t, 4, True, False, backend="hip", fused_step=True)


def _net():
    return construct_mlp(5, 1, [8], ["ELU"], None)


def _two_groups(net):
    ps = list(net.parameters())
    return torch.optim.Adam([{"params": ps[:2]}, {"params": ps[2:]}], lr=1e-3)


@pytest.mark.parametrize("make_opt, named", [
    (lambda net: torch.optim.SGD(net.parameters(), lr=0.1), "TRAIN.OPTIMIZER.cls SGD"),
    (lambda net: torch.optim.Adamax(net.parameters()), "TRAIN.OPTIMIZER.cls Adamax"),
    (lambda net: torch.optim.Adam(net.parameters(), amsgrad=True), "amsgrad"),
    (lambda net: torch.optim.AdamW(net.parameters(), maximize=True), "maximize"),
    (lambda net: torch.optim.Adam(net.parameters(), capturable=True), "capturable"),
    (lambda net: torch.optim.Adam(net.parameters(), differentiable=True), "differentiable"),
    (lambda net: torch.optim.Adam(net.parameters(), lr=torch.tensor(1e-3)), "tensor lr"),
    (_two_groups, "2 param groups"),
    (lambda net: torch.optim.Adam(list(net.parameters())[:2]), "param group"),
], ids=["sgd", "adamax", "amsgrad", "maximize", "capturable", "differentiable", "tensor_lr", "two_groups",
        "other_params"])
def test_optimizer_refusals_at_the_first_batch(make_opt, named):
    """No GPU and no library: the optimizer is checked before either is touched."""
    step = fit.device_step(0.0, torch.square, fit.FixedLossScaler(1.0), 4)
    net = _net()
    before = [p.detach().clone() for p in net.parameters()]
    with pytest.raises(NotImplementedError, match=named) as e:
        step(net, make_opt(net), torch.zeros(3, 5), torch.zeros(3, 5))
    assert "TRAIN.FUSED_STEP" in str(e.value)
    assert all(torch.equal(a, p) for a, p in zip(before, net.parameters()))


@pytest.mark.parametrize("make, named", [
    (lambda: PISGradNet([16], 4, lambda x: x.sum(-1, keepdim=True)), "TRAIN.FUSED_STEP with NETWORK.PISGRADNET"),
    (lambda: construct_mlp(5, 1, [8, 8], ["ELU", "Tanh"], None), "TRAIN.BACKEND: hip with NETWORK.ACTIVATIONS"),
    (lambda: construct_mlp(5, 1, [8], ["ELU"], 3.0), "TRAIN.BACKEND: hip with NETWORK.BOUND"),
    (lambda: construct_mlp(5, 5, [8], ["ELU"], None), "gradient head"),
    (lambda: construct_mlp(5, 1, [8], ["ELU"], None).double(), "float64"),
    (lambda: construct_mlp(5, 1, [300], ["ELU"], None), "TRAIN.BACKEND: hip with NETWORK.NEURONS"),
], ids=["pisgradnet", "mixed_activations", "bound", "head", "fp64", "width"])
def test_network_refusals_at_the_first_batch(make, named):
    """A PISGradNet is refused by TRAIN.FUSED_STEP; what _DevicePlan refuses keeps its text."""
    step = fit.device_step(0.0, torch.square, fit.FixedLossScaler(1.0), 4)
    net = make()
    with pytest.raises(NotImplementedError, match=named):
        step(net, torch.optim.Adam(net.parameters()), torch.zeros(3, 5), torch.zeros(3, 5))


def test_state_is_created_as_torch_creates_it_and_nothing_falls_back():
    """A CPU batch is an error, not a torch step; the optimizer state the check created before it has torch's
    layout: a CPU scalar `step` of 0, zero moments like the parameters, and state_dict() takes it."""
    from deeppicarditeration_amd import _lib
    from deeppicarditeration_amd.build import build
    build(verbose=False)
    step = fit.device_step(0.0, torch.square, fit.FixedLossScaler(1.0), 4)
    net = _net()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in net.parameters()]
    with pytest.raises(_lib.DPIError, match="no CPU fallback"):
        step(net, opt, torch.zeros(3, 5), torch.zeros(3, 5))
    assert all(torch.equal(a, p) and p.grad is None for a, p in zip(before, net.parameters()))
    ref = torch.optim.AdamW(_net().parameters(), lr=1e-3)
    for p in ref.param_groups[0]["params"]:
        p.grad = torch.zeros_like(p)
    ref.step()
    for p, q in zip(opt.param_groups[0]["params"], ref.param_groups[0]["params"]):
        st, want = opt.state[p], ref.state[q]
        assert set(st) == set(want) and float(st["step"]) == 0.0
        for k in want:
            assert st[k].dtype == want[k].dtype and st[k].device == want[k].device and st[k].shape == want[k].shape
        assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
