"""Time the general MLP family on GBM (csrc/dpi_general_gbm.h) beside its yardstick.

The GBM bench shape (bench.py --workload gbm, configs[4]) — GBMEquationComplexExact, nx = 100, SDGD
v = 100, 64 points x 1,024 paths, K = 50 — one label step = sample_with_gradients (points, per-point
baseline, path launches, reduce).  Per net: warm-up calls, then REPS calls each bracketed by its own pair
of HIP events; the median is reported (ms/step), with the minimum beside it.  The yardstick is the
specialised 3 x 64 instance in DPI_GEMM_F32 (the same arithmetic: exact-fp32 MFMA) and in the default
mode, in the same process on the same device; then the new family at 4 x 64, 5 x 64, 8 x 64, 4 x 32 and
[40].  `scaled_yardstick_ms`: the fp32 yardstick times the ratio of the network-phase FLOPs (the tangent
sweep over 100 directions dominates: per direction 2 MACs-as-FLOPs per padded hidden weight).  One JSON
line per net, and the LDS / register figures of the new kernels from the library's code objects.

    python tools/time_gbm_deep.py [--reps 30] [--warmup 5] [--act ELU]
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

NX, V, N, M, K = 100, 100, 64, 1024, 50
NETS = [("specialised 3x64 fp32", [64] * 3, L.DPI_GEMM_F32), ("specialised 3x64 auto", [64] * 3, L.DPI_GEMM_AUTO),
        ("general 4x64", [64] * 4, None), ("general 5x64", [64] * 5, None), ("general 8x64", [64] * 8, None),
        ("general 4x32", [32] * 4, None), ("general 1x40", [40], None)]


def pad(w):  # the padded width the kernels compute with: a multiple of 32 (16 for the specialised H = 16)
    return (w + 31) // 32 * 32


def sweep_flops(widths):
    """FLOPs per path of the network phase: forward and adjoint passes (layer 1 over nx) and the tangent
    sweep, 2 FLOPs per padded hidden weight and direction."""
    p = [pad(w) for w in widths]
    hidden = sum(a * b for a, b in zip(p[:-1], p[1:]))
    return 2 * (NX * p[0] + 2 * hidden) + 2 * NX * hidden + 3 * NX * sum(p)


def time_net(widths, mode, act, reps, warmup):
    torch.manual_seed(0)
    eq = dpi.GBMEquationComplexExact(NX, 1.0, 1.0)
    net = dpi.construct_mlp(1 + NX, 1, widths, [act] * len(widths), None)
    gen = dpi.OnlineDataGenerator(eq, net, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=M,
                                  n_estimate_integral=M, n_euler_steps=K, seed=5,
                                  hessian_approximation={"method": "SDGD", "kwargs": {"v": V}})
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
            "ms_median": t[len(t) // 2], "ms_min": t[0], "net_mflop_per_path": sweep_flops(widths) / 1e6,
            "workspace_mb": gen.workspace_bytes(N, M) / 2 ** 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--act", default="ELU", choices=["ELU", "Tanh"])
    a = ap.parse_args()
    assert a.reps >= 20, "the median of at least 20 calls"
    for k in kernel_resources():
        if any(f in k["name"] for f in ("k_paths_gbm_gen<", "k_baseline_gbm_gen<")):
            print(json.dumps({"kernel": k["name"].split("(")[0], "vgpr": k["vgpr_count"], "agpr": k["agpr_count"],
                              "lds_bytes": k["group_segment_fixed_size"], "sgpr_spill": k["sgpr_spill_count"],
                              "vgpr_spill": k["vgpr_spill_count"]}), flush=True)
    yard = None
    for name, widths, mode in NETS:
        r = time_net(widths, mode, a.act, a.reps, a.warmup)
        if yard is None:
            yard = (r["ms_median"], r["net_mflop_per_path"])
        r["scaled_yardstick_ms"] = yard[0] * r["net_mflop_per_path"] / yard[1]
        print(json.dumps({"net": name, "act": a.act, **r}), flush=True)


if __name__ == "__main__":
    main()
