"""Time one optimizer step of the fit — objective, backward and Adam step — under both fit backends
(DESIGN.md §5.1): the device objective (TRAIN.BACKEND: hip, csrc/dpi_fit.h) and the torch objective it
bypasses, in one process on one device, alternating, PAIRS runs each.

Four shapes: the shipped Burgers fit (B = 512, nx = 100, 4 x 128 ELU, c = 1), the shape of the r03c
`picard train` log (B = 128, nx = 8, [32, 32] ELU, c = 0.1), and two PISGradNet fits on an OUProcessEquation with
a seeded two-component mixture: the HJB YAML's (B = 512, nx = 100, [512] * 4, c = 0.1) and the nest YAML's
(B = 512, nx = 10, [64] * 4, c = 1).  Per run: warm-up steps, then REPS steps each
bracketed by its own pair of HIP events; the median is reported (ms/step) with the minimum beside it.  One
JSON line per run, then one per shape with the acceptance figures of the project's protocol (§2.1): every
device run below every torch run, and the gain against 3 x the spread of the torch runs.

    python tools/time_fit.py [--reps 30] [--warmup 5] [--pairs 3] [--only SUBSTRING]

--step-forms times, by the same protocol, the two forms of a step under TRAIN.BACKEND: hip for the two
construct_mlp shapes: "fused" (TRAIN.FUSED_STEP: fit.device_step, loss, gradients and the Adam update in
dpi_fit_step's two launches) against "unfused" (the device objective, backward and torch's Adam), the
baseline; --form fused|unfused runs that one form alone once per shape (for a kernel trace).

--core-form tiles|layers (TRAIN.CORE_FORM) times, for the two PISGradNet shapes, the device objective with that
form of the core against torch; with --against-tiles, "layers" against "tiles" instead, alternating in the
same way; with --form-alone, that form alone once per shape (for a kernel trace).

--pis-shell hip (TRAIN.PIS_SHELL), with --core-form: the device objective with the shell in HIP ("shell-hip": the
time networks, the g0 part and the loss from dpi_fit_shell_*) against the same core form with the shell in torch
("shell-torch", the baseline); with --form-alone, "shell-hip" alone once per shape.
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import deeppicarditeration_amd as dpi  # noqa: E402
from deeppicarditeration_amd import fit  # noqa: E402

SHAPES = [("burgers B512 nx100 4x128 ELU c1", 512, 100, [128] * 4, 1.0),
          ("r03c B128 nx8 2x32 ELU c0.1", 128, 8, [32, 32], 0.1),
          ("hjb pisgradnet B512 nx100 4x512 c0.1", 512, 100, [512] * 4, 0.1),
          ("nest pisgradnet B512 nx10 4x64 c1", 512, 10, [64] * 4, 1.0)]


def make_net(name, nx, widths):
    if "pisgradnet" not in name:
        return dpi.construct_mlp(1 + nx, 1, widths, ["ELU"] * len(widths), None)
    eq = dpi.OUProcessEquation(nx=nx, T=1.0, num_components=2, mean=torch.randn(2, nx, dtype=torch.float64),
                               var=2.0 * torch.ones(2, nx, dtype=torch.float64),
                               pi=torch.tensor([0.4, 0.6], dtype=torch.float64))
    return dpi.PISGradNet(hidden_shapes=list(widths), dim=nx, g0=eq.g, T=1.0)


def time_steps(name, backend, B, nx, widths, c, reps, warmup, core_form=None):
    torch.manual_seed(0)
    net = make_net(name, nx, widths).to("cuda")
    scaler = fit.FixedLossScaler(c)
    make = {"hip": fit.device_objective, "unfused": fit.device_objective, "fused": fit.device_step,
            "torch": fit.gradient_objective, "tiles": fit.device_objective, "layers": fit.device_objective,
            "shell-hip": fit.device_objective, "shell-torch": fit.device_objective}[backend]
    form = {"core_form": backend} if backend in ("tiles", "layers") else {}
    if backend.startswith("shell-"):
        form = {"core_form": core_form, "pis_shell": backend[len("shell-"):]}
    objective = make(0.0, torch.square, scaler, nx, **form)
    steps = fit.fused_train_steps if backend == "fused" else fit.train_steps
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    tx = torch.cat([torch.rand(B, 1), torch.randn(B, nx)], 1).to("cuda")
    y = (torch.randn(B, 1 + nx) * 0.5).to("cuda")
    batch = [(tx, y)]
    for _ in range(warmup):
        steps(net, objective, opt, batch)
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        losses = steps(net, objective, opt, batch)
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all()
    t = sorted(a.elapsed_time(b) for a, b in evs)
    return {"ms_median": t[len(t) // 2], "ms_min": t[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--only", default="", help="time the shapes whose name contains this")
    ap.add_argument("--step-forms", action="store_true", help="time the fused step against the unfused hip step")
    ap.add_argument("--form", choices=("fused", "unfused"), default=None, help="run this step form alone, once")
    ap.add_argument("--core-form", choices=("tiles", "layers"), default=None,
                    help="the PISGradNet shapes with this form of the core (TRAIN.CORE_FORM) against torch")
    ap.add_argument("--against-tiles", action="store_true", help="with --core-form layers: against tiles, not torch")
    ap.add_argument("--form-alone", action="store_true", help="with --core-form: run that form alone, once")
    ap.add_argument("--pis-shell", choices=("hip",), default=None,
                    help="with --core-form: the shell in HIP (TRAIN.PIS_SHELL) against the shell in torch, same core form")
    a = ap.parse_args()
    assert a.reps >= 20, "the median of at least 20 steps"
    forms = a.step_forms or a.form is not None
    core = a.core_form is not None
    assert not (core and forms), "--core-form is for the PISGradNet shapes, --step-forms / --form for the others"
    assert core or not (a.against_tiles or a.form_alone), "--against-tiles and --form-alone go with --core-form"
    assert not a.against_tiles or a.core_form == "layers", "--against-tiles compares layers with tiles"
    new, old = ("fused", "unfused") if forms else ("hip", "torch")
    if core:
        new, old = a.core_form, "tiles" if a.against_tiles else "torch"
    alone = a.form if a.form is not None else (a.core_form if a.form_alone else None)
    assert core or a.pis_shell is None, "--pis-shell goes with --core-form"
    assert not (a.pis_shell and a.against_tiles), "--pis-shell compares the shells, --against-tiles the core forms"
    if a.pis_shell:
        new, old = "shell-hip", "shell-torch"
        alone = new if a.form_alone else None
    for name, B, nx, widths, c in [s for s in SHAPES if a.only in s[0] and not (forms and "pisgradnet" in s[0])
                                   and not (core and "pisgradnet" not in s[0])]:
        if alone is not None:
            r = time_steps(name, alone, B, nx, widths, c, a.reps, a.warmup, a.core_form)
            print(json.dumps({"shape": name, "backend": alone, **r}), flush=True)
            continue
        runs = {new: [], old: []}
        for _ in range(a.pairs):
            for backend in (new, old):
                r = time_steps(name, backend, B, nx, widths, c, a.reps, a.warmup, a.core_form)
                runs[backend].append(r["ms_median"])
                print(json.dumps({"shape": name, "backend": backend, **r}), flush=True)
        spread = max(runs[old]) - min(runs[old])
        gain = min(runs[old]) - max(runs[new])
        print(json.dumps({"shape": name, f"{new}_ms": runs[new], f"{old}_ms": runs[old],
                          f"every_{new}_run_faster": max(runs[new]) < min(runs[old]), "gain_ms": gain,
                          f"{old}_spread_ms": spread, "gain_over_3_spreads": gain > 3 * spread,
                          f"ratio_{old}_over_{new}": [min(runs[old]) / max(runs[new]),
                                                      max(runs[old]) / min(runs[new])]}), flush=True)


if __name__ == "__main__":
    main()
