"""Time the general MLP family (csrc/dpi_general.h) beside its yardstick.

The Burgers bench shape — Cha, nx = 100, 16 points x 4,096 paths, K = 50 — one label step =
sample_with_gradients (points, per-point baseline, path launches, reduce).  Per net: warm-up calls,
then REPS calls each bracketed by its own pair of HIP events; the median is reported (ms/step), with
the minimum beside it.  The yardstick is the specialised 4 x 128 instance in both precision modes,
in the same process on the same device; then the general 4 x 64, 5 x 128, 8 x 128, 4 x 256, 8 x 256.
One JSON line per net, and the LDS / register / workgroups-per-CU figures of the general kernels
from the library's code objects.

    python tools/time_general_mlp.py [--reps 30] [--warmup 5] [--act ELU]
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
        ("general 4x256", [256] * 4, None), ("general 8x256", [256] * 8, None)]


def mlp_flops(widths):
    """Forward + backward MACs x 2 per path of the padded network phase (layer 1 over nx)."""
    f = 2 * NX * widths[0] + sum(2 * 2 * a * b for a, b in zip(widths[:-1], widths[1:]))
    return 2 * f


def time_net(widths, mode, act, reps, warmup):
    torch.manual_seed(0)
    eq = dpi.Cha(NX, 1.0, 5.0, 1.0)
    net = dpi.construct_mlp(1 + NX, 1, widths, [act] * len(widths), None)
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
    return {"family": "general" if family == L.DPI_FAMILY_GENERAL else "specialised", "ms_median": t[len(t) // 2],
            "ms_min": t[0], "mlp_mflop_per_path": mlp_flops(widths) / 1e6, "stash_slots": gen.net.general_slots(),
            "workspace_mb": gen.workspace_bytes(N, M) / 2 ** 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--act", default="ELU", choices=["ELU", "Tanh"])
    a = ap.parse_args()
    assert a.reps >= 20, "the median of at least 20 calls"
    for k in kernel_resources():
        if "k_paths_gen<" in k["name"] or "k_baseline_gen<" in k["name"]:
            print(json.dumps({"kernel": k["name"].split("(")[0], "vgpr": k["vgpr_count"], "agpr": k["agpr_count"],
                              "lds_bytes": k["group_segment_fixed_size"], "sgpr_spill": k["sgpr_spill_count"],
                              "vgpr_spill": k["vgpr_spill_count"]}), flush=True)
    for name, widths, mode in NETS:
        print(json.dumps({"net": name, "act": a.act, **time_net(widths, mode, a.act, a.reps, a.warmup)}), flush=True)


if __name__ == "__main__":
    main()
