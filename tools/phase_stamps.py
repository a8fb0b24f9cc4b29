"""Reduce the phase stamps of the parking path kernels (csrc/dpi_device.h DPI_PHASE_STAMPS) on the
flagship shape: Burgers configs[1], 16 points x 4,096 paths, K = 50, one k_paths_fb launch of 1,024
path blocks.

The stamps exist only in the diagnostic build:
    python tools/build_variant.py stamps --units dpi_paths_fb_cha.hip -DDPI_PHASE_STAMPS=1
    DPI_HIP_LIB=tools/variants/libdpi_stamps.so python tools/phase_stamps.py --order 0 --out FILE.json
(--order: the DPI_ORDER of the stamped launch; 4 is the all-terminal-last schedule every split launch
ran before the park.  --tail: its DPI_TAIL — the tail units of csrc/dpi_tail_units.h; default: the
library's rule; 0: whole blocks.)  Every wave of a path block stores s_memtime (shader cycles) at its phase
boundaries into the block's park row, and wave 0 its HW_ID / XCC_ID and the block's order.  The
counters of different CUs are not aligned (they read up to 2e8 cycles apart inside one XCD), so
stamps are compared within a CU only, and a CU's times are taken from its first block's start: the
1,040 workgroups of the launch start within a microsecond of each other.  Printed and written as JSON:
  - mlp: per CU, how much of the residents' MLP phases ran while the co-resident block was in its own
    MLP phase (overlap_fraction: that time over all MLP time);
  - barrier_wait: cycles a wave waits at the barrier after its last rollout before the MLP, and at the
    one after the terminal rollout (terminal-last) / the reload (terminal-first), mean and slowest wave;
  - mlp_start_gap: how far apart the two residents of a CU enter their MLP phases, per round;
  - tail: the time from the first workgroup slot going idle to the last one (each from its CU's first start);
  - pairs: per round, the CUs whose two residents ran opposite orders.
With tail units a split block is stamped twice — its T-unit in wave 0's last dim-block of the park row, its
I-unit in wave 1's, word [1] carrying the role — and the unit that does not finish the block leaves stamps
5-7 unwritten.  The reduction is then by workgroup, not by block: how many units of each kind, which kind
finished, a unit's cycles to its join, and the same tail figures (a slot is busy to the last stamp of its
last workgroup).
The stamped build's run time is not the product's: read the shares, not the length."""
import argparse
import collections
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import deeppicarditeration_amd as dpi  # noqa: E402
from deeppicarditeration_amd import _lib as L  # noqa: E402

N, M, K, NX = 16, 4096, 50, 100
ROW_WORDS = 4 * 8 * 64 * 4 * 4 // 8  # a park row in 64-bit words
STAMP_WORD = 7 * 64 * 4 * 4 // 8     # the row's stamp area: wave 0's last dim-block
UNIT_WORD = 8 * 64 * 4 * 4 // 8      # an I-unit's stamp area: the same dim-block of wave 1, this much further
WHOLE, I_UNIT, T_UNIT = 1, 2, 3      # dpi_tail_units.h TailRole, in bits 8.. of word [1]


def stamped_launch(order, tail=None):
    torch.manual_seed(0)
    net = dpi.construct_mlp(1 + NX, 1, [128] * 4, ["ELU"] * 4, None)
    gen = dpi.OnlineDataGenerator(dpi.Cha(NX, 1.0, 5.0, 1.0), net, 1, 1, device="cuda:0", t_always_uniform=True,
                                  n_estimate_terminal=M, n_estimate_integral=M, n_euler_steps=K, seed=1)
    os.environ["DPI_ORDER"] = str(order)
    if tail is not None:
        os.environ["DPI_TAIL"] = str(tail)
    for _ in range(50):  # warm: clocks and caches as in a running bench
        gen.sample_generate(N, 0)
    ws = gen._workspace(N, M)
    rows = N * M // 64
    p0 = gen.workspace_bytes(N, M) - L.DPI_PARK_MAX_BLOCKS * ROW_WORDS * 8  # the park: the workspace's last region
    park = ws[p0:p0 + rows * ROW_WORDS * 8]
    park.zero_()
    gen.sample_generate(N, 0)
    torch.cuda.synchronize()
    words = park.cpu().numpy().view(np.uint64).reshape(rows, ROW_WORDS).astype(np.int64)
    return np.stack([words[:, STAMP_WORD + a * UNIT_WORD:STAMP_WORD + a * UNIT_WORD + 36] for a in (0, 1)], 1)


def idle_times(key, slot, start, end):
    """Per workgroup slot, when it went idle: its last workgroup's end, from its CU's first start."""
    by_cu = collections.defaultdict(list)
    for b in range(len(start)):
        by_cu[key[b]].append(b)
    idle = []
    for items in by_cu.values():
        t0, last = min(int(start[b]) for b in items), collections.defaultdict(int)
        for b in items:
            last[int(slot[b])] = max(last[int(slot[b])], int(end[b]) - t0)
        idle += list(last.values())
    idle.sort()
    return len(by_cu), {"workgroup_slots": len(idle), "first_slot_idle_at": idle[0], "tenth_slot_idle_at": idle[len(idle) // 10],
                        "quarter_slot_idle_at": idle[len(idle) // 4], "median_slot_idle_at": idle[len(idle) // 2],
                        "last_slot_idle_at": idle[-1], "tail_cycles": idle[-1] - idle[0],
                        "tail_fraction": (idle[-1] - idle[0]) / idle[-1]}


def reduce_units(w2):
    """The launch by workgroup: whole blocks and the T- and I-units of the split ones."""
    w = w2.reshape(-1, 36)
    w = w[w[:, 4] > 0]  # stamped areas: wave 0's first stamp
    t = w[:, 4:36].reshape(-1, 4, 8)
    role = (w[:, 1] >> 8) & 0xFF
    hw = w[:, 0] & 0xFFFFFFFF
    key = list(zip(((w[:, 0] >> 32) & 0xF).tolist(), ((hw >> 13) & 7).tolist(), ((hw >> 12) & 1).tolist(),
                   ((hw >> 8) & 0xF).tolist()))
    start, end, fin = t[:, :, 0].min(1), t.reshape(len(t), -1).max(1), t[:, 0, 7] > 0
    out = {"blocks": int(len(w2)), "whole_blocks": int((role == WHOLE).sum()), "t_units": int((role == T_UNIT).sum()),
           "i_units": int((role == I_UNIT).sum()), "finished_by_t_unit": int((fin & (role == T_UNIT)).sum()),
           "finished_by_i_unit": int((fin & (role == I_UNIT)).sum())}
    for name, r, k in (("t_unit_cycles_to_join_mean", T_UNIT, 1), ("i_unit_cycles_to_join_mean", I_UNIT, 4)):
        sel = role == r
        if sel.any():
            out[name] = float((t[sel][:, :, k].max(1) - start[sel]).mean())
            f = sel & fin
            if f.any():
                out[name.replace("cycles_to_join", "finisher_cycles_after_join")] = float((end[f] - t[f][:, :, k].max(1)).mean())
    if (role == WHOLE).any():
        out["whole_block_cycles_mean"] = float((end - start)[role == WHOLE].mean())
    out["cus"], out["tail"] = idle_times(key, (hw >> 16) & 0xF, start, end)
    return out


def overlap(a, b):
    return max(0, min(a[1], b[1]) - max(a[0], b[0]))


def reduce(w2):
    if (((w2[:, :, 1] >> 8) & 0xFF) >= I_UNIT).any():
        return reduce_units(w2)
    w = w2[:, 0]
    t = w[:, 4:36].reshape(-1, 4, 8)  # [block][wave][stamp]
    if not (t[:, :, 0] > 0).all():
        raise SystemExit("no stamps in the park: is DPI_HIP_LIB the -DDPI_PHASE_STAMPS=1 variant?")
    hw = w[:, 0] & 0xFFFFFFFF
    xcc, cu, sh, se, slot = (w[:, 0] >> 32) & 0xF, (hw >> 8) & 0xF, (hw >> 12) & 1, (hw >> 13) & 7, (hw >> 16) & 0xF
    tlast = (w[:, 1] & 1) != 0
    start, end = t[:, :, 0].min(1), t[:, :, 7].max(1)
    mlp = np.stack([t[:, :, 3].min(1), t[:, :, 4].max(1)], 1)
    out = {"blocks": int(len(w)), "terminal_last_blocks": int(tlast.sum()),
           "block_cycles_mean": float((end - start).mean()), "mlp_cycles_mean": float((mlp[:, 1] - mlp[:, 0]).mean())}
    # the barrier after the last rollout before the MLP (stamp 2 -> 3; lane 0 of wave 0 polls the base record
    # there) and after the terminal rollout or the reload (5 -> 6)
    wait_mlp, wait_term = t[:, :, 3] - t[:, :, 2], t[:, :, 6] - t[:, :, 5]
    out["barrier_wait"] = {"before_mlp_mean": float(wait_mlp.mean()), "before_mlp_by_wave": wait_mlp.mean(0).tolist(),
                           "after_terminal_mean_terminal_last": float(wait_term[tlast].mean()) if tlast.any() else None,
                           "after_terminal_by_wave_terminal_last": wait_term[tlast].mean(0).tolist() if tlast.any() else None,
                           "after_reload_mean_terminal_first": float(wait_term[~tlast].mean()) if (~tlast).any() else None}
    # a wave's own rollouts (means over waves and blocks), by the block's order
    for name, sel, (i0, i1), (t0_, t1_) in (("terminal_last", tlast, (0, 2), (4, 5)), ("terminal_first", ~tlast, (1, 2), (0, 1))):
        if sel.any():
            out[f"rollout_cycles_mean_{name}"] = {"integral": float((t[sel][:, :, i1] - t[sel][:, :, i0]).mean()),
                                                  "terminal": float((t[sel][:, :, t1_] - t[sel][:, :, t0_]).mean())}
    by_cu = collections.defaultdict(list)
    for b in range(len(w)):
        by_cu[(int(xcc[b]), int(se[b]), int(sh[b]), int(cu[b]))].append(b)
    both, total, rounds, gaps, idle = 0, 0, collections.defaultdict(lambda: [0, 0]), collections.defaultdict(list), []
    for blocks in by_cu.values():
        blocks.sort(key=lambda b: start[b])
        total += sum(int(mlp[b, 1] - mlp[b, 0]) for b in blocks)
        for x, a in enumerate(blocks):
            for b in blocks[x + 1:]:
                both += 2 * int(overlap(mlp[a], mlp[b]))
        t0, last = int(start[blocks[0]]), collections.defaultdict(int)
        for b in blocks:
            last[int(slot[b])] = max(last[int(slot[b])], int(end[b]) - t0)
        idle += list(last.values())
        for r in range(0, len(blocks) - 1, 2):  # residents of round r / 2: the r-th and (r + 1)-th block to start
            a, b = blocks[r], blocks[r + 1]
            if overlap((start[a], end[a]), (start[b], end[b])) > 0:
                rounds[r // 2][0] += 1
                rounds[r // 2][1] += int(tlast[a] != tlast[b])
                gaps[r // 2].append(abs(int(mlp[a, 0]) - int(mlp[b, 0])))
    out["cus"] = len(by_cu)
    out["mlp"] = {"cycles_total": total, "cycles_beside_a_resident_in_its_mlp": both,
                  "overlap_fraction": both / max(total, 1)}
    out["pairs"] = {f"round_{r}": {"co_resident_pairs": v[0], "in_opposite_orders": v[1]} for r, v in sorted(rounds.items())}
    out["mlp_start_gap"] = {f"round_{r}": {"mean": float(np.mean(v)), "min": int(min(v))} for r, v in sorted(gaps.items())}
    idle.sort()
    out["tail"] = {"workgroup_slots": len(idle), "first_slot_idle_at": idle[0], "tenth_slot_idle_at": idle[len(idle) // 10], "quarter_slot_idle_at": idle[len(idle) // 4],
                   "median_slot_idle_at": idle[len(idle) // 2],
                   "last_slot_idle_at": idle[-1], "tail_cycles": idle[-1] - idle[0], "tail_fraction": (idle[-1] - idle[0]) / idle[-1]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--order", type=int, default=0)
    ap.add_argument("--tail", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"shape": f"Cha nx={NX}, MLP 4x128 ELU fp16-split, {N} points x {M} paths, K={K}: k_paths_fb, "
                    f"{N * M // 64} path blocks", "DPI_ORDER": a.order, "DPI_TAIL": "default" if a.tail is None else a.tail,
           "unit": "shader cycles (s_memtime)", **reduce(stamped_launch(a.order, a.tail))}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
