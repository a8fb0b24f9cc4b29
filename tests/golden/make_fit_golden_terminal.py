"""Golden vectors for the outer fit of terminal-enforcing solutions (NETWORK.cls
PicardSolutionEnforceTerminal) from the REFERENCE's training steps, written to
tests/golden/fit_terminal/*.npz (a folder of its own: tests/test_fit_golden.py takes every fit_*.npz
under tests/golden/fit/ for a plain value network).

Runs only where the reference is present (the module stand-ins and the package bypass are
make_golden.py's, the configuration nodes make_fit_golden.py's).  Each case builds the reference's own
PicardSolutionEnforceTerminal (picard/solution_enforce_terminal.py:9-27) in fp64, wraps it in
PicardSolutionGradientWrapper (solution_jac.py:112-136, whose construct_solution takes
runner.get_solution_plain()) and runs S optimizer steps of its training_step (solution_jac.py:167-213) on
fixed batches: the objectives are computed on the wrapper's forward, g + (T - t) N.  Stored: the
configuration, initial weights, batches, per-step losses and final weights (data only).

Usage:  python tests/golden/make_fit_golden_terminal.py
"""
import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_fit_golden as mf  # noqa: E402  (imports make_golden: the stand-ins and the reference)

mg, sj, CfgNode = mf.mg, mf.sj, mf.CfgNode
set_mod = importlib.import_module("picard.solution_enforce_terminal")
OUT = HERE / "fit_terminal"

CASES = {
    # name: (nx, neurons, act, TYPE, beta, scaler (cls, kwargs) | None, loss-fn clip | None)
    "fit_term_v_fixed": (12, [16, 16], "ELU", "Value", 0.5, ("FixedLossScaler", {"fixed_weight": 0.1}), None),
    "fit_term_og_fixed": (12, [16, 16], "Tanh", "OnlyGradient", 0.5, ("FixedLossScaler", {"fixed_weight": 0.3}), None),
    "fit_term_og_default_scaler_clip": (9, [24, 24, 24], "ELU", "OnlyGradient", 0.0, None, 0.5),
}
S, B, LR = mf.S, mf.B, mf.LR


def run(name):
    nx, neurons, act, typ, beta, scaler, clip = CASES[name]
    torch.set_default_dtype(torch.float64)
    eq = mg.eqs.Cha(nx, 1.0, 5.0, 1.0)
    tcfg = mf.train_cfg(beta, scaler, clip, -1)
    ncfg = CfgNode({"TYPE": typ, "PISGRADNET": False, "NEURONS": neurons, "ACTIVATIONS": [act] * len(neurons),
                    "BOUND": None})
    torch.manual_seed(sum(map(ord, name)))
    plain = set_mod.PicardSolutionEnforceTerminal(eq, ncfg, tcfg)

    class Runner:  # the parts of PicardRunner construct_solution reads
        def get_solution_plain(self):
            return plain

    model = sj.PicardSolutionGradientWrapper.construct_solution(Runner())
    init = {k: v.detach().clone().numpy() for k, v in plain.model.state_dict().items()}
    g = torch.Generator().manual_seed(13)
    tx = torch.cat([torch.rand(S, B, 1, generator=g), torch.randn(S, B, nx, generator=g)], -1)
    y = 0.5 * torch.randn(S, B, 1 + nx, generator=g)
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    losses = []
    for s in range(S):
        loss = model.training_step((tx[s], y[s]), s)
        opt.zero_grad()
        loss.sum().backward()
        opt.step()
        losses.append(float(loss.sum()))
    final = {k: v.detach().numpy() for k, v in plain.model.state_dict().items()}
    cfg = {"nx": nx, "neurons": neurons, "act": act, "type": typ, "output_dim": int(plain.output_dim), "beta": beta,
           "scaler": scaler, "clip": clip, "lr": LR, "wrapped": type(model).__name__, "cls": type(plain).__name__,
           "eq": {"nx": nx, "alpha": 1.0, "k": 5.0, "T": 1.0}}
    out = {"cfg": np.array(json.dumps(cfg)), "tx": tx.numpy(), "y": y.numpy(), "losses": np.array(losses)}
    out.update({f"init.{k}": v for k, v in init.items()})
    out.update({f"final.{k}": v for k, v in final.items()})
    OUT.mkdir(exist_ok=True)
    np.savez_compressed(OUT / f"{name}.npz", **out)
    print(name, cfg["wrapped"], cfg["cls"], losses)


if __name__ == "__main__":
    for n in (sys.argv[1:] or CASES):
        run(n)
