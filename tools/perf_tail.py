"""Ablation of the tail units (DPI_TAIL, DPI_TAIL_ORDER) on the Burgers bench shape's k_paths launch:
interleaved rounds in one process, medians, and the moments compared bitwise with the first variant.
usage: perf_tail.py sweep [tail:order ...]     16 points x 4096 paths (1,024 blocks)
       perf_tail.py fb [tail:order ...]        the same shape as the one-launch k_paths_fb (sample_generate)
       perf_tail.py rounds [tail ...]          4 / 8 / 16 / 24 / 32 points (256 ... 2,048 blocks);
                                               a tail of "default" leaves DPI_TAIL unset"""
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tools.perf_probe import bench, make  # noqa: E402
from deeppicarditeration_amd import _lib as L  # noqa: E402

ROUNDS = int(os.environ.get("PERF_ROUNDS", "7"))


def set_tail(tail, order="0"):
    if tail == "default":
        os.environ.pop("DPI_TAIL", None)
    else:
        os.environ["DPI_TAIL"] = tail
    os.environ["DPI_TAIL_ORDER"] = order


def bench_fb(gen, n, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        gen.sample_generate(n, 0)
    e0.record()
    for _ in range(reps):
        gen.sample_generate(n, 0)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(objs, variants, M=4096, fb=False):
    gen, tx, ws = objs
    res, moms = {v: [] for v in variants}, {}
    for _ in range(ROUNDS):
        for v in variants:
            set_tail(*v)
            if fb:
                res[v].append(bench_fb(gen, tx.shape[0]))
                moms[v] = gen.sample_generate(tx.shape[0], 0)[1].clone()
            else:
                res[v].append(bench(gen, tx, ws, L.DPI_BOTH, M))
                moms[v] = gen.label_moments(tx, 0, M, 0, M, L.DPI_BOTH, ws).clone()
    torch.cuda.synchronize()
    out = {}
    for v in variants:
        t = sorted(res[v])
        out[v] = (t[len(t) // 2] * 1e3, t[0] * 1e3, (t[-1] - t[0]) * 1e3, bool(torch.equal(moms[v], moms[variants[0]])))
    return out


def main():
    mode, args = sys.argv[1], sys.argv[2:]
    L.load()
    if mode in ("sweep", "fb"):
        variants = [tuple(a.split(":")) for a in args] or [("0", "0")] + [
            (t, o) for t in ("128", "256", "384", "512", "768", "1024") for o in ("0", "1")]
        out = run(make("128x4", 50), variants, fb=mode == "fb")
        base = out[variants[0]][0]
        for v in variants:
            med, lo, spread, same = out[v]
            print(f"tail={v[0]:>7s} order={v[1]}  median {med:7.1f} us  min {lo:7.1f} us  spread {spread:5.1f} us  "
                  f"gain {100 * (base - med) / base:5.2f} %  bits {'same' if same else 'DIFFER'}", flush=True)
    else:
        tails = args or ["0", "default"]
        for n in (4, 8, 16, 24, 32):
            out = run(make("128x4", 50, n=n), [(t, "0") for t in tails])
            base = out[(tails[0], "0")][0]
            line = f"n={n:3d} blocks={n * 64:5d} rounds={n * 64 / 512:4.1f}"
            for t in tails:
                med, lo, spread, same = out[(t, "0")]
                line += f"  tail={t:>7s} {med:7.1f} us spread {spread:4.1f} gain {100 * (base - med) / base:5.2f} %" + \
                    ("" if same else " BITS DIFFER")
            print(line, flush=True)


if __name__ == "__main__":
    main()
