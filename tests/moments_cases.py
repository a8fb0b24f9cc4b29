"""The case table and helpers of tests/test_moments_reference.py (CPU) and tests/test_gpu_moments.py (MI355X):
the label moments (sum of c, sum of c^2 over the Monte-Carlo paths, c the per-path contribution whose mean
is the label) against the fp64 oracle, entry by entry.

A case is a row of tests/net_weight_cases.py (its net, scales, equation; n = 3, K = 2, seed 1, epoch 1) plus
the entry point the call goes through, the estimator flags and, where it differs, the path count M.  One
row per code path that writes or reduces the second half of `moments`.

The metrics, for the fp64 reference S1 = sum c, S2 = sum c^2 over the M paths a call summed:
    e1 = |S1' - S1| / sqrt(M S2)     the error of the mean in units of the entry's per-path rms
    e2 = |S2' - S2| / S2
(the Hessian sums likewise, in the scale sqrt(M sum h^2)).

`restate` is a numpy restatement of how the moments are formed from the per-path pieces, with the faults of
FAULTS one at a time: the mutant gate of test_moments_reference.py shows that each fault moves sum c^2 by
>= 1e-3 in e2 wherever a case reaches its edge, and by exactly 0.0 where it cannot."""
from collections import namedtuple

import numpy as np

import net_weight_cases as T
import terminal_util as TU
from oracle import dpi_oracle as O

BLOCK = 64
TERMINAL, INTEGRAL, BOTH = 1, 2, 3

# name: the test id; c: the net_weight_cases.Case (M overridden where the row asks); entry: the call
# (generate / finalize / moments / sample / ranges / prepared / hess); flags: the estimators; base: the id
# of the row in net_weight_cases.SCALES whose scales the net takes; terminal: (equation, type, act, widths
# tag, nx) of a terminal-enforcing net of tests/terminal_util.py instead of a net_weight_cases net
MCase = namedtuple("MCase", "name c entry flags base terminal")

_BY_ID = {T.case_id(c): c for c in T.CASES}


def _row(case_id, entry="generate", flags=BOTH, M=None, tag=None):
    c = _BY_ID[case_id]
    base = T.net_id(c)
    if M is not None:
        c = c._replace(M=M)
    name = case_id + (f"-M{M}" if M is not None else "") + ("-" + tag if tag else "") + "-" + entry
    return MCase(name, c, entry, flags, base, None)


def _build():
    rows = []
    # paths_body, the 56-column form: [32, 32] at nx = 7, plain and TD, ELU in both GEMM modes, Tanh once
    rows += [_row("unit-cha-ELU-2x32-nx7-f32"), _row("unit-cha-ELU-2x32-nx7-auto", "finalize"),
             _row("unit-ou-ELU-2x32-nx7-f32", "finalize"), _row("unit-ou-ELU-2x32-nx7-auto"),
             _row("unit-gbm-ELU-2x32-nx7-f32"), _row("unit-gbm-ELU-2x32-nx7-auto", "finalize"),
             # Tanh with OU: at the cha Tanh row's second point f_b (T - t) is 2e-2 of the value column's rms and
             # `baseline_outside_square` moves sum c^2 by 3.6e-4 only, under the mutant gate's floor
             _row("unit-ou-Tanh-2x32-nx7-auto"),
             _row("unit-cha-ELU-2x32-nx7-td-auto"), _row("unit-ou-ELU-2x32-nx7-td-f32"),
             _row("unit-gbm-ELU-2x32-nx7-td-auto", "finalize")]
    for mode in ("f32", "auto"):
        rows += [_row(f"edge-cha-ELU-4x128-nx100-{mode}"), _row(f"edge-ou-ELU-3x64-nx100-{mode}")]
        # the eighth dim-block: one dim in it, and full
        rows += [_row(f"edge-cha-ELU-2x64-nx113-{mode}"), _row(f"edge-cha-ELU-2x64-nx128-{mode}")]
    # the wide instances (nx = 129: groups of seven)
    rows += [_row(f"unit-{eq}-ELU-2x32-nx129-wide-auto") for eq in ("cha", "ou", "gbm")]
    # the per-lane baseline (GBM with SDGD)
    rows += [_row("edge-gbm-ELU-3x64-nx100-v100-auto"), _row("edge-gbm-ELU-3x64-nx100-v7-auto"),
             _row("edge-gbm-ELU-3x64-nx100-v7-f32", "finalize")]
    # the general family, the gradient heads, a terminal-enforcing net
    rows += [_row(f"general-{eq}-ELU-{w}-nx7-auto") for eq in ("cha", "ou") for w in ("1x40", "129x200x256")]
    rows += [_row("head-cha-ELU-1x40-nx7-ValueGradient-auto"), _row("head-ou-ELU-1x40-nx7-OnlyGradient-auto")]
    tc = ("cha", "Value", "ELU", "w40", 7)
    rows.append(MCase("terminal-" + TU.case_id(tc) + "-generate",
                      T._case("general", "cha", "ELU", TU.WIDTHS["w40"], 7, "auto"), "generate", BOTH, None, tc))
    # PISGradNet: the layer-wise chain ([32, 32]) and the fused one ([512]), both modes; TD once
    for mode in ("f32", "auto"):
        rows += [_row(f"pis-ou-ELU-2x32-nx100-{mode}"), _row(f"pis-ou-ELU-1x512-nx100-{mode}")]
    rows.append(_row("pis-ou-ELU-4x512-nx100-td-auto"))
    # dead lanes: M = 100 (28 of the second block's lanes), M = 1 (63 of 64)
    rows += [_row("edge-cha-ELU-4x128-nx100-M100-auto"), _row("edge-ou-ELU-3x64-nx100-M100-auto"),
             _row("edge-gbm-ELU-3x64-nx100-M100-v100-auto"), _row("unit-cha-ELU-2x32-nx7-auto", M=1)]
    # one estimator alone
    for cid in ("unit-cha-ELU-2x32-nx7-auto", "edge-gbm-ELU-3x64-nx100-v7-auto"):
        rows += [_row(cid, "moments", TERMINAL, tag="terminal"), _row(cid, "moments", INTEGRAL, tag="integral")]
    # the reducers, cha [16] at nx = 7: in-launch (two blocks), k_reduce (65 blocks), dpi_moments_reduce
    rows += [_row("unit-cha-ELU-1x16-nx7-f32", "moments"), _row("unit-cha-ELU-1x16-nx7-f32", "moments", M=4160),
             _row("unit-cha-ELU-1x16-nx7-f32", "ranges")]
    # the one-launch hand-off, the prepared pairs
    rows += [_row("unit-cha-ELU-2x32-nx7-fb-auto", "sample"), _row("unit-ou-ELU-2x32-nx7-fb-auto", "sample"),
             _row("pis-ou-ELU-2x32-nx100-auto", "prepared"), _row("edge-gbm-ELU-3x64-nx100-v7-auto", "prepared")]
    # Hessian labels
    rows += [_row(f"hess-gbm-ELU-2x32-nx7-{mode}", "hess") for mode in ("f32", "auto")]
    assert len({r.name for r in rows}) == len(rows)
    return rows


CASES = _build()


def delta_t(mc):
    return T.DT if mc.c.variant == "td" else 0.0


def ref_id(mc):
    """What the fp64 reference depends on: the net, the path count, the estimators."""
    net = "terminal-" + TU.case_id(mc.terminal) if mc.terminal else mc.base
    return net + ("" if f"-M{mc.c.M}" in net else f"-M{mc.c.M}") + f"-flags{mc.flags}"


def ref_cases():
    """One case per reference (the GEMM modes and entry points of one net share it)."""
    seen = {}
    for mc in CASES:
        seen.setdefault(ref_id(mc), mc)
    return list(seen.values())


def build(mc):
    """(product equation, oracle equation, module, oracle twin) of the case."""
    if mc.terminal:
        from deeppicarditeration_amd.solution import PicardSolutionEnforceTerminal
        eq_kind, kind, act, wtag, nx = mc.terminal
        eq, oeq = TU.equation(eq_kind, nx)
        inner, acts = TU.case_nets(*mc.terminal)
        return eq, oeq, PicardSolutionEnforceTerminal(eq, inner, kind), TU.from_module(oeq, inner, acts, kind)
    eq, oeq = T.equations(mc.c)
    module, onet = T.network(mc.c, eq, oeq, T.SCALES[mc.base])
    return eq, oeq, module, onet


# ----------------------------------------------------------------------------- the fp64 reference
def e1(s1, S1, S2, M):
    return np.abs(np.asarray(s1, np.float64) - S1) / np.sqrt(M * S2)


def e2(s2, S2):
    return np.abs(np.asarray(s2, np.float64) - S2) / S2


def device_order_f32(rows, m_begin=0):
    """Sum of fp32 rows (paths, C), the first of them path m_begin (a multiple of 64), in the device's
    order: O.tree_sum_f32 per 64-path block (a partial last block padded with +0), then over the blocks."""
    assert m_begin % BLOCK == 0
    rows = np.asarray(rows, np.float32)
    blocks = [rows[b:b + BLOCK] for b in range(0, rows.shape[0], BLOCK)]
    return O.tree_sum_f32(np.stack([O.tree_sum_f32(b) for b in blocks]))


# S1, S2 (n, 1+nx), H1, H2 (n, nx^2; None without Hessian labels), g (n,): the fp64 sums of path_moments;
# yard: the CPU yardstick at these points, the largest e1 / e2 (/ eh: e1 of the Hessian sums) of the same
# rows rounded to fp32, squared and summed in fp32 in the device's order
Ref = namedtuple("Ref", "S1 S2 H1 H2 g yard")
_REFERENCES = {}


def reference(mc, oeq, onet, tx, m_begin=0, m_end=None):
    """The Ref of the case at points tx over the paths [m_begin, m_end) (default: all M), computed once
    per reference and points, read-only."""
    tx = np.asarray(tx, np.float64)
    m_end = mc.c.M if m_end is None else m_end
    key = (ref_id(mc), tx.tobytes(), m_begin, m_end)
    if key not in _REFERENCES:
        Mc = m_end - m_begin
        cols, yard = [], {"e1": 0.0, "e2": 0.0}
        for r in range(tx.shape[0]):
            out = O.path_moments(oeq, onet, tx[r], r, m_begin, m_end, T.K, T.SEED, T.EPOCH, delta_t=delta_t(mc),
                                 flags=mc.flags, v=mc.c.v, hessians=mc.c.hess, return_rows=True)
            if mc.c.hess:
                S1, S2, H1, H2, g, c, h = out
                yard["eh"] = max(yard.get("eh", 0.0), e1(device_order_f32(h, m_begin), H1, H2, Mc).max())
            else:
                (S1, S2, g, c), H1, H2 = out, None, None
            c32 = c.astype(np.float32)
            yard["e1"] = max(yard["e1"], e1(device_order_f32(c32, m_begin), S1, S2, Mc).max())
            yard["e2"] = max(yard["e2"], e2(device_order_f32(c32 * c32, m_begin), S2).max())
            cols.append((S1, S2, H1, H2, g))
        arrs = [None if col[0] is None else np.stack(col) for col in zip(*cols)]
        for a in arrs:
            if a is not None:
                a.setflags(write=False)
        _REFERENCES[key] = Ref(*arrs, yard)
    return _REFERENCES[key]


# ----------------------------------------------------------------------------- per-path pieces (CPU tests)
Pieces = namedtuple("Pieces", "cT cI base live c h g")


def pieces(mc, oeq, onet, tx_row, ig):
    """The per-path pieces of one point over every launched lane (M rounded up to whole 64-path blocks):
    cT (flags = 1) and cI (flags = 2, without the baseline term) (lanes, 1+nx), the baseline term
    f_b (T - t) per lane (zero where the case's flags leave the integral estimator out), the live mask
    m < M, and the oracle's own rows c (the case's flags), h (Hessian labels, else None) and g(x)."""
    M = mc.c.M
    m = np.arange(-(-M // BLOCK) * BLOCK)

    def rows(flags):
        if mc.c.hess:
            c, h, g, b = O.path_contributions_hess(oeq, onet, tx_row, ig, m, T.K, T.SEED, T.EPOCH, flags=flags,
                                                   return_baseline=True)
            return c, h, g, b
        c, g, b = O.path_contributions(oeq, onet, tx_row, ig, m, T.K, T.SEED, T.EPOCH, delta_t=delta_t(mc),
                                       flags=flags, v=mc.c.v, return_baseline=True)
        return c, None, g, b

    zero = np.zeros((len(m), 1 + oeq.nx))
    cT = rows(TERMINAL)[0] if mc.flags & TERMINAL else zero
    base = np.zeros(len(m))
    cI = zero
    if mc.flags & INTEGRAL:
        cI, _, _, base = rows(INTEGRAL)
        cI = cI.copy()
        cI[:, 0] -= base
    c, h, g, _ = rows(mc.flags)
    return Pieces(cT, cI, base, m < M, c, h, g)


FAULTS = ("parts_squared_apart", "square_of_block_sum", "baseline_outside_square", "dead_lanes_counted",
          "last_dim_lost", "eighth_block_swapped", "block_lost")
EIGHTH = 112  # dims d >= 112 are the eighth dim-block of paths_body's phase 3


def restate(p, fault=None):
    """(S1, S2) (1+nx,) of one point from its pieces, in fp64: c = cT + cI (+ the baseline term in the
    value column) on the live lanes, 0 on the dead ones; every square per lane, then the sums.  `fault`:
    one of FAULTS."""
    assert fault is None or fault in FAULTS
    live = p.live[:, None]
    tfull = np.where(live, p.cT, 0.0)
    ifull = np.where(live, p.cI, 0.0)
    ifull[:, 0] += np.where(p.live, p.base, 0.0)
    c = tfull + ifull
    S1, S2 = c.sum(0), (c * c).sum(0)
    if fault == "parts_squared_apart":
        S2 = (tfull * tfull).sum(0) + (ifull * ifull).sum(0)
    elif fault == "square_of_block_sum":
        bs = c.reshape(-1, BLOCK, c.shape[1]).sum(1)
        S2 = (bs * bs).sum(0) / BLOCK
    elif fault == "baseline_outside_square":
        nb = c.copy()  # summed as the faultless columns are, so that a zero baseline moves exactly nothing
        nb[:, 0] = tfull[:, 0] + np.where(p.live, p.cI[:, 0], 0.0)
        S2 = (nb * nb).sum(0)
    elif fault == "dead_lanes_counted":
        dead = np.where(p.live, 0.0, p.base)
        S2[0] = S2[0] + (dead * dead).sum()
    elif fault == "last_dim_lost":
        S2[-1] = 0.0
    elif fault == "eighth_block_swapped":
        S1, S2 = S1.copy(), S2.copy()
        S1[1 + EIGHTH:], S2[1 + EIGHTH:] = S2[1 + EIGHTH:].copy(), S1[1 + EIGHTH:].copy()
    elif fault == "block_lost":
        S2 = (c[:BLOCK] * c[:BLOCK]).sum(0)
    return S1, S2


def touched(fault, nx):
    """The columns of sum c^2 a fault can move."""
    if fault in ("baseline_outside_square", "dead_lanes_counted"):
        return [0]
    if fault == "last_dim_lost":
        return [nx]
    if fault == "eighth_block_swapped":
        return list(range(1 + EIGHTH, 1 + nx))
    return list(range(1 + nx))


def reached(fault, mc, nx):
    """Whether the case reaches the fault's edge (by its shape alone; the gate shows the rest)."""
    M = mc.c.M
    return {"parts_squared_apart": mc.flags == BOTH,
            "square_of_block_sum": True,
            "baseline_outside_square": bool(mc.flags & INTEGRAL),
            "dead_lanes_counted": bool(mc.flags & INTEGRAL) and M % BLOCK != 0,
            "last_dim_lost": True,
            "eighth_block_swapped": nx > EIGHTH,
            "block_lost": M > BLOCK}[fault]
