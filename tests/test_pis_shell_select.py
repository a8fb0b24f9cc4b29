"""TRAIN.PIS_SHELL and what it selects (config.py, fit.build_objective, fit.device_objective) — CPU only, no
library.  "torch", the default, builds what was built before the key existed; "hip", under TRAIN.BACKEND: hip,
hands a PISGradNet's whole objective to `_PISShell`, and what it does not cover is refused by name: at
configuration load where the configuration shows it, otherwise at the first batch before the library is touched."""
import pytest
import torch

import pis_fit_reference as R
from deeppicarditeration_amd import _lib, fit
from deeppicarditeration_amd.config import get_default_cfg, load_cfg
from deeppicarditeration_amd.solution import PISGradNet, construct_mlp


def _yaml(tmp_path, train=""):
    f = tmp_path / "a.yaml"
    f.write_text(f"NAME: x\nTRAIN: {{{train}}}\n")
    return str(f)


def _eq(nx=4):
    return R.make_equation((3, nx, [16], 1.0, 0.0, False, 1.0))


def test_key_defaults_to_torch_and_loads(tmp_path):
    assert get_default_cfg().TRAIN.PIS_SHELL == "torch"
    assert load_cfg(_yaml(tmp_path)).TRAIN.PIS_SHELL == "torch"
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip")).TRAIN.PIS_SHELL == "torch"
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip, PIS_SHELL: hip")).TRAIN.PIS_SHELL == "hip"
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip"), ["TRAIN.PIS_SHELL", "hip"]).TRAIN.PIS_SHELL == "hip"
    assert load_cfg(_yaml(tmp_path), ["TRAIN.BACKEND", "hip", "TRAIN.PIS_SHELL", "hip"]).TRAIN.PIS_SHELL == "hip"
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip, PIS_SHELL: hip"), ["TRAIN.PIS_SHELL", "torch"]).TRAIN.PIS_SHELL == "torch"
    assert load_cfg(_yaml(tmp_path, "PIS_SHELL: torch")).TRAIN.PIS_SHELL == "torch"  # the default under torch too
    cfg = load_cfg(_yaml(tmp_path, "BACKEND: hip, PIS_SHELL: hip, CORE_FORM: layers"))
    assert (cfg.TRAIN.PIS_SHELL, cfg.TRAIN.CORE_FORM) == ("hip", "layers")
    for bad in ("HIP", "kernels", "1"):
        with pytest.raises(ValueError, match="TRAIN.PIS_SHELL"):
            load_cfg(_yaml(tmp_path, f"BACKEND: hip, PIS_SHELL: {bad}"))


def test_hip_under_the_torch_backend_is_refused_at_load(tmp_path):
    for train in ("PIS_SHELL: hip", "BACKEND: torch, PIS_SHELL: hip"):
        with pytest.raises(NotImplementedError, match="TRAIN.PIS_SHELL") as e:
            load_cfg(_yaml(tmp_path, train))
        assert "TRAIN.BACKEND: torch" in str(e.value)
    with pytest.raises(NotImplementedError, match="TRAIN.PIS_SHELL") as e:
        fit.build_objective(get_default_cfg().TRAIN, 4, True, False, backend="torch", pis_shell="hip")
    assert "TRAIN.BACKEND: torch" in str(e.value)
    with pytest.raises(ValueError, match="TRAIN.PIS_SHELL"):
        fit.build_objective(get_default_cfg().TRAIN, 4, True, False, backend="hip", pis_shell="kernels")
    with pytest.raises(ValueError, match="TRAIN.PIS_SHELL"):
        fit.device_objective(0.0, torch.square, None, 4, pis_shell="kernels")


def test_build_objective_hands_the_option_to_the_device_objective(monkeypatch):
    """The same closure and kinds; the option arrives at `_PISPlan` beside the core's form, which then holds the
    shell's table in state-dict order.  The CPU batch is then the error: nothing falls back to torch."""
    t = get_default_cfg().TRAIN
    seen = []
    plan_cls = fit._PISPlan

    class Plan(plan_cls):
        def __init__(self, *args):
            seen.append(args[2:])
            super().__init__(*args)

    monkeypatch.setattr(fit, "_PISPlan", Plan)
    net = PISGradNet([16, 16], 4, _eq().g)
    for form in ("tiles", "layers"):
        for sg, want in ((False, "value"), (True, "gradient")):
            obj, kind = fit.build_objective(t, 4, sg, False, backend="hip", core_form=form, pis_shell="hip")
            assert kind == want and obj.__qualname__.startswith("device_objective.")
        with pytest.raises(_lib.DPIError, match="no CPU fallback"):
            obj(net, torch.zeros(3, 5), torch.zeros(3, 5))
    assert seen == [("tiles", "hip"), ("layers", "hip")]
    plan = plan_cls(net, 4, "layers", "hip")
    assert plan.pis_shell == "hip" and plan.shell_ws is None and plan.ws is None
    names = ["timestep_phase"] + [f"t_encoder.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")]
    names += [f"smooth_net.{2 * j}.{w}" for j in range(4) for w in ("weight", "bias")]
    params = dict(net.named_parameters())
    assert len(plan.shell_params) == len(names) and all(p is params[n] for p, n in zip(plan.shell_params, names))
    assert {id(p) for p in plan.shell_params + plan.params} == {id(p) for p in net.parameters()}
    assert plan_cls(net, 4).pis_shell == "torch" and not hasattr(plan_cls(net, 4), "shell_params")

    eq = _eq()  # an equation object without dpi_problem(): refused by name
    stub = type("OUProcessEquation", (), {"g": lambda self, x: eq.g(x)})()
    with pytest.raises(NotImplementedError, match="dpi_problem"):
        plan_cls(PISGradNet([16], 4, stub.g), 4, "tiles", "hip")


def test_a_construct_mlp_net_under_hip_is_refused_by_name_at_the_first_batch(monkeypatch):
    """No GPU and no library: the network is looked at before either is touched, and no parameter is."""
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was touched"))
    net = construct_mlp(5, 1, [8, 8], ["ELU", "ELU"], None)
    before = [p.detach().clone() for p in net.parameters()]
    for form in ("tiles", "layers"):
        obj = fit.device_objective(0.0, torch.square, fit.FixedLossScaler(1.0), 4, core_form=form, pis_shell="hip")
        with pytest.raises(NotImplementedError, match="TRAIN.PIS_SHELL") as e:
            obj(net, torch.zeros(3, 5), torch.zeros(3, 5))
        assert "hip" in str(e.value) and "PISGradNet" in str(e.value) and "Sequential" in str(e.value)
    step = fit.device_step(0.0, torch.square, fit.FixedLossScaler(1.0), 4, pis_shell="hip")
    with pytest.raises(NotImplementedError, match="TRAIN.PIS_SHELL"):
        step(net, torch.optim.Adam(net.parameters()), torch.zeros(3, 5), torch.zeros(3, 5))
    assert all(torch.equal(p, b) and p.grad is None for p, b in zip(net.parameters(), before))
    # the fused step with a PISGradNet keeps its own refusal
    pis = PISGradNet([16], 4, _eq().g)
    with pytest.raises(NotImplementedError, match="TRAIN.FUSED_STEP with NETWORK.PISGRADNET"):
        step(pis, torch.optim.Adam(pis.parameters()), torch.zeros(3, 5), torch.zeros(3, 5))


def test_the_default_builds_what_it_built_before(monkeypatch):
    """No pis_shell, or "torch": device_objective is called with today's arguments and `_PISPlan` with today's
    three."""
    calls, seen = [], []
    real, plan_cls = fit.device_objective, fit._PISPlan

    def recording(*args, **kwargs):
        calls.append((len(args), kwargs))
        return real(*args, **kwargs)

    class Plan(plan_cls):
        def __init__(self, *args):
            seen.append(len(args))
            super().__init__(*args)

    monkeypatch.setattr(fit, "device_objective", recording)
    monkeypatch.setattr(fit, "_PISPlan", Plan)
    t = get_default_cfg().TRAIN
    net = PISGradNet([16], 4, _eq().g)
    for shell in ({}, {"pis_shell": "torch"}):
        obj, kind = fit.build_objective(t, 4, True, False, backend="hip", **shell)
        assert kind == "gradient"
        with pytest.raises(_lib.DPIError, match="no CPU fallback"):
            obj(net, torch.zeros(3, 5), torch.zeros(3, 5))
    assert calls == [(4, {}), (4, {})] and seen == [3, 3]
