"""Find the (hidden, out) scales of tests/net_weight_cases.py SCALES on the CPU with the fp64 oracle.

For every net of the case table: over hidden in {1, 2, 4, 8, 16} and out in {1/64, ..., 1, 2, ..., 4096}, keep
the candidates that pass tests/net_weight.py's gate with a margin (shares in [0.052, 0.94], mutants >= 1.1e-3:
the GPU tests gate at the device's fp32 points, the CPU test at the oracle's fp64 ones), and print the one
whose shares lie deepest inside the band (largest min over blocks of min(log(s / 0.05), log(0.95 / s))),
as a line of the SCALES literal.  No device is needed.

    python tools/search_net_weight.py [-j PROCESSES] [--seeds 17,18,...] [--cases MODULE] [substring of the net ids]

--cases MODULE: another case module under tests/ with net_weight_cases' interface (CASES, net_id, equations,
network, oracle_kw, N, SEED, EPOCH), for instance gbm_deep_cases."""
import importlib
import math
import os
import sys
from multiprocessing import Pool

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # one thread per worker process
    os.environ.setdefault(_v, "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

LO, HI, FLOOR = 0.052, 0.94, 1.1e-3
SEEDS = [17]
CASES = ["net_weight_cases"]


def cases_module():
    return importlib.import_module(CASES[0])


def search(c):
    for seed in SEEDS:
        nid, best = search_seed(c, seed)
        if best is not None:
            break
    return nid, best, seed


def search_seed(c, seed):
    import numpy as np
    import torch

    import net_weight as NW
    from oracle import dpi_oracle as O
    T = cases_module()
    torch.set_num_threads(1)
    eq, oeq = T.equations(c)
    tx = O.sample_points(oeq, T.N, T.SEED, T.EPOCH, 0)
    kw = T.oracle_kw(c)
    hess_nx = oeq.nx if c.hess else None
    zero = None
    best = None
    for h in (1, 2, 4, 8, 16):
        for e in range(-6, 13):
            o = 2.0 ** e if e < 0 else 2 ** e
            _, onet = T.network(c, eq, oeq, (h, o, seed))
            ref = NW.labels(oeq, onet, tx, **kw)
            if not np.isfinite(ref).all():
                break
            if zero is None or c.pis:
                zero = NW.labels(oeq, NW.without_network(onet), tx, **kw)
            sh = NW.blocks(zero, ref, hess_nx)
            if min(sh.values()) > HI:
                break
            if not all(LO <= s <= HI for s in sh.values()):
                continue
            eff = {n: NW.blocks(NW.labels(oeq, m, tx, **kw), ref, hess_nx) for n, m in NW.mutants(onet)}
            live = {n: max(e_.values()) for n, e_ in eff.items() if any(x != 0.0 for x in e_.values())}
            if min(live.values()) < FLOOR:
                continue
            score = min(min(math.log(s / 0.05), math.log(0.95 / s)) for s in sh.values())
            if best is None or score > best[0]:
                best = (score, h, o, sh, min(live, key=live.get), min(live.values()),
                        sorted(set(eff) - set(live)), float(np.abs(ref).max()))
    return T.net_id(c), best


def _init(seeds, cases):  # the workers' copies of the options (a spawned worker re-imports this module)
    SEEDS[:] = seeds
    CASES[:] = cases


def main():
    args = sys.argv[1:]
    jobs = int(args[args.index("-j") + 1]) if "-j" in args else 8
    if "--seeds" in args:  # net seeds to try in turn where 17 gives no candidate
        SEEDS[:] = [int(x) for x in args[args.index("--seeds") + 1].split(",")]
    if "--cases" in args:
        CASES[:] = [args[args.index("--cases") + 1]]
    T = cases_module()
    flags = ("-j", "--seeds", "--cases")
    pats = [a for i, a in enumerate(args) if a not in flags and (i == 0 or args[i - 1] not in flags)]
    nets = {}
    for c in T.CASES:
        if not pats or any(p in T.net_id(c) + "$" for p in pats):  # 'nx7$' ends an id
            nets.setdefault(T.net_id(c), c)
    with Pool(jobs, _init, (list(SEEDS), list(CASES))) as pool:
        for nid, best, seed in pool.imap(search, list(nets.values())):
            if best is None:
                print(f"    # {nid!r}: NO CANDIDATE PASSES", flush=True)
                continue
            _, h, o, sh, weakest, eff, exempt, mx = best
            shares = " / ".join(f"{s:.3f}" for s in sh.values())
            note = f"share {shares}; weakest mutant {weakest} {eff:.1e}" + (f"; exempt {', '.join(exempt)}" if exempt else "")
            tail = "" if seed == 17 else f", {seed}"
            print(f"    {nid!r}: ({h}, {o}{tail}),  # {note}; max |label| {mx:.1e}", flush=True)


if __name__ == "__main__":
    main()
