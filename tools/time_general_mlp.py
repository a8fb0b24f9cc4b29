"""Time the general MLP family (csrc/dpi_general.h) beside its yardstick.

The Burgers bench shape — Cha, nx = 100, 16 points x 4,096 paths, K = 50 — one label step =
sample_with_gradients (points, per-point baseline, path launches, reduce).  Per net: warm-up calls,
then REPS calls each bracketed by its own pair of HIP events; the median is reported (ms/step), with
the minimum beside it.  The yardstick is the specialised 4 x 128 instance in both precision modes,
in the same process on the same device; then the general 4 x 64, 5 x 128, 8 x 128, 4 x 256, 8 x 256,
and the gradient-head nets (NETWORK.TYPE ValueGradient / OnlyGradient) 4 x 128 and
8 x 256, which run the general family's forward-only head kernels.  One JSON line per net, and the LDS / register / workgroups-per-CU figures of the general kernels
from the library's code objects.

--ansatz: the terminal-enforcing solutions (NETWORK.cls PicardSolutionEnforceTerminal)
instead — Cha and OU at nx = 100, [64] * 4 and [128] * 4: the plain Value and OnlyGradient routes (the
yardsticks, in the same process) beside the terminal-enforcing Value and OnlyGradient forms.

    python tools/time_general_mlp.py [--reps 30] [--warmup 5] [--act ELU] [--ansatz]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import deeppicarditeration_amd as dpi  # noqa: E402
from deeppicarditeration_amd import _lib as L  # noqa: E402
from deeppicarditeration_amd.build import kernel_resources  # noqa: E402

NX, N, M, K = 100, 16, 4096, 50
NETS = [("specialised 4x128 fp16-split", [128] * 4, L.DPI_GEMM_AUTO), ("specialised 4x128 fp32", [128] * 4, L.DPI_GEMM_F32),
        ("general 4x64", [64] * 4, None), ("general 5x128", [128] * 5, None), ("general 8x128", [128] * 8, None),
        ("general 4x256", [256] * 4, None), ("general 8x256", [256] * 8, None),
        ("head 4x128 ValueGradient", [128] * 4, None, 1 + NX), ("head 4x128 OnlyGradient", [128] * 4, None, NX),
        ("head 8x256 ValueGradient", [256] * 8, None, 1 + NX), ("head 8x256 OnlyGradient", [256] * 8, None, NX)]


def mlp_flops(widths, n_out=1):
    """Forward + backward MACs x 2 per path of the padded network phase (layer 1 over nx); a gradient
    head (n_out > 1): the forward MACs and the output rows (Cha reads only their sum: two dots)."""
    if n_out > 1:
        return 2 * (NX * widths[0] + sum(a * b for a, b in zip(widths[:-1], widths[1:])) + 2 * widths[-1])
    f = 2 * NX * widths[0] + sum(2 * 2 * a * b for a, b in zip(widths[:-1], widths[1:]))
    return 2 * f


def equation(kind):
    if kind == "cha":
        return dpi.Cha(NX, 1.0, 5.0, 1.0)
    return dpi.OUProcessEquation(nx=NX, T=1.0, alpha=1.0, num_components=5, mean_scale=1.0, var_scale=2.0, alpha_scale=4.0)


def time_net(widths, mode, act, reps, warmup, n_out=1, eq_kind="cha", ansatz=False):
    torch.manual_seed(0)
    eq = equation(eq_kind)
    net = dpi.construct_mlp(1 + NX, n_out, widths, [act] * len(widths), None)
    if ansatz:
        net = dpi.PicardSolutionEnforceTerminal(eq, net, "Value" if n_out == 1 else "OnlyGradient")
    gen = dpi.OnlineDataGenerator(eq, net, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=M,
                                  n_estimate_integral=M, n_euler_steps=K, seed=5)
    if mode is not None:
        gen.net.set_precision(mode)
    family = gen.net.family(gen.problem)
    for _ in range(warmup):
        _, y = gen.sample_with_gradients(N)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        gen.sample_with_gradients(N)
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in evs)
    return {"family": "general" if family == L.DPI_FAMILY_GENERAL else "specialised", "desc": gen.net.desc,
            "ms_median": t[len(t) // 2],
            "ms_min": t[0], "mlp_mflop_per_path": mlp_flops(widths, n_out) / 1e6, "stash_slots": gen.net.general_slots(),
            "workspace_mb": gen.workspace_bytes(N, M) / 2 ** 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--act", default="ELU", choices=["ELU", "Tanh"])
    ap.add_argument("--ansatz", action="store_true", help="the terminal-enforcing forms beside their plain routes")
    a = ap.parse_args()
    assert a.reps >= 20, "the median of at least 20 calls"
    names = ("k_paths_term<", "k_baseline_term<", "k_paths_head_term<", "k_baseline_head_term<") if a.ansatz else \
        ("k_paths_gen<", "k_baseline_gen<", "k_paths_head<", "k_baseline_head<")
    for k in kernel_resources():
        if any(f in k["name"] for f in names):
            print(json.dumps({"kernel": k["name"].split("(")[0], "vgpr": k["vgpr_count"], "agpr": k["agpr_count"],
                              "lds_bytes": k["group_segment_fixed_size"], "sgpr_spill": k["sgpr_spill_count"],
                              "vgpr_spill": k["vgpr_spill_count"]}), flush=True)
    if a.ansatz:
        for eq_kind in ("cha", "ou"):
            for widths in ([64] * 4, [128] * 4):
                for n_out in (1, NX):
                    for ansatz in (False, True):
                        typ = "Value" if n_out == 1 else "OnlyGradient"
                        name = f"{eq_kind} {len(widths)}x{widths[0]} {typ}" + (" terminal" if ansatz else " plain")
                        print(json.dumps({"net": name, "act": a.act,
                                          **time_net(widths, None, a.act, a.reps, a.warmup, n_out, eq_kind, ansatz)}),
                              flush=True)
        return
    for name, widths, mode, *n_out in NETS:
        print(json.dumps({"net": name, "act": a.act, **time_net(widths, mode, a.act, a.reps, a.warmup, *n_out)}),
              flush=True)


if __name__ == "__main__":
    main()
