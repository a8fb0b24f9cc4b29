"""The tail units of the parking path kernels (csrc/dpi_device.h paths_body, csrc/dpi_tail_units.h; DPI_TAIL).

A launch may run its last path blocks as two workgroups each: a T-unit (terminal rollout; hands over ST and
its g statistics) and an I-unit (integral rollout and MLP; hands over the noise tile and bsh).  Whichever
arrives second at the block's join word finishes the block.  The split decides who does the work and
when, never what is computed, so every policy gives the bits of the whole-block launch (DPI_TAIL=0):

  DPI_TAIL         1, an odd count (3) and all blocks (a count above the cap)
  DPI_TAIL_ORDER   0 I-units then T-units, 1 T-units then I-units
  DPI_TAIL_LAUNCHES=2  the second units as a launch of their own behind the first on the stream: with
                   order 0 every block is finished by its T-unit, with order 1 by its I-unit — both
                   finisher paths run for certain, without a wait
  crossed with DPI_ORDER 0 and 4 (the whole blocks' phase order)

for k_paths (gen.label_moments) and k_paths_fb (dpi_sample_with_gradients where the pair has one).
Shapes as tests/test_gpu_phase_order.py, plus nx = 128 (a park row without an unused dim-block slot: two
extra rows per split block).  OU's gst has five statistics per wave; OU 4 x 128 ELU parks nothing and has
no units: equal because untouched.  The single-estimator flags take the unsplit path.

Equal bits alone would also hold if no unit ever ran, so every call is followed by dpi_launch_units (the
split count, grid and launch count of the thread's last path launch) against what the policy asks for:
the units ran where they should, and nowhere else.  OU's units in k_paths_fb need a net that kernel is
instantiated for (not 4 x 128): a 2 x 64 ELU case.  A label call captured into a graph carries one join
sequence through every replay: replays with the points changed in between must give the eager labels."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import noise_table_cases as C
import test_gpu_phase_order as PO
import deeppicarditeration_amd as dpi
from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd import data as D

N, PB = PO.N, PO.PB
# (DPI_TAIL, DPI_TAIL_ORDER, DPI_TAIL_LAUNCHES); the first is the reference
POLICIES = [("0", "0", "1")] + [(t, o, l) for t in ("1", "3", "100000") for o in ("0", "1") for l in ("1", "2")]
ORDERS = ("0", "4")


def _set(monkeypatch, policy, order="0"):
    for k, v in zip(("DPI_TAIL", "DPI_TAIL_ORDER", "DPI_TAIL_LAUNCHES"), policy):
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DPI_ORDER", order)


def _units():
    """(split blocks, grid, launches) of this thread's last k_paths / k_paths_fb launch."""
    t, g, n = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    L.check(L.load().dpi_launch_units(ctypes.byref(t), ctypes.byref(g), ctypes.byref(n)), "dpi_launch_units")
    return t.value, g.value, n.value


def _expected_units(policy, flags, nblk, nbase, has_units=True):
    """What the policy asks of a call of nblk path blocks (all of them fit the park's free rows here)."""
    tail = min(int(policy[0]), nblk) if has_units and flags == L.DPI_BOTH else 0
    return tail, nbase + nblk + tail, 2 if tail and policy[2] == "2" else 1


def _compare(gen, has_units, fb, M, K, monkeypatch, flag_set):
    """Every policy x DPI_ORDER against DPI_TAIL=0, k_paths and (fb) k_paths_fb, with the launches' units."""
    nblk = N * ((M + 63) // 64)
    tx, _ = gen.sample_t_and_x(N, point_base=PB)
    ws = gen.point_baseline(tx)
    for flags in flag_set:
        want = None
        # the single-estimator flags run whole blocks whatever the policy says: two policies do
        for policy in POLICIES if flags == L.DPI_BOTH else (POLICIES[0], POLICIES[-1], POLICIES[-4]):
            for order in ORDERS:
                _set(monkeypatch, policy, order)
                mom = gen.label_moments(tx, PB, M, 0, M, flags, ws)
                assert _units() == _expected_units(policy, flags, nblk, 0, has_units), (M, K, flags, policy)
                got = (mom,) + PO._sample(gen, N, PB, flags)
                assert _units() == _expected_units(policy, flags, nblk, N if fb else 0, has_units), (M, K, flags, policy)
                torch.cuda.synchronize()
                assert all(torch.isfinite(g).all() for g in got)
                want = got if want is None else want
                for g, w in zip(got, want):
                    assert torch.equal(g, w), (M, K, flags, policy, order)
        assert torch.equal(want[1], tx) and torch.equal(want[0], want[3])


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [100, 7, 128])
@pytest.mark.parametrize("act", ["ELU", "Tanh"])
@pytest.mark.parametrize("kind", ["cha", "ou"])
def test_labels_do_not_depend_on_the_tail_units(kind, act, nx, monkeypatch):
    for M in (128, 100):
        for K in (3, 70):
            gen = PO._generator(kind, act, False, nx, M, K)
            # k_paths_fb: ELU nets, not OU 4 x 128 (else dpi_sample_with_gradients is baseline + k_paths)
            # and OU 4 x 128 ELU has no units
            _compare(gen, (kind, act) != ("ou", "ELU"), (kind, act) == ("cha", "ELU"), M, K, monkeypatch, PO.FLAGS)


def _small_generator(kind, nx, M, K):
    """A 2 x 64 ELU net: a pair k_paths_fb is instantiated for with OU, too."""
    torch.manual_seed(nx + 1000 * K)
    net = dpi.construct_mlp(1 + nx, 1, [64] * 2, ["ELU"] * 2, None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", D.PartialBlockNote)
        return dpi.OnlineDataGenerator(PO._equation(kind, nx), net, 1, 1, device="cuda:0", t_always_uniform=True,
                                       n_estimate_terminal=M, n_estimate_integral=M, n_euler_steps=K, seed=PO.SEED,
                                       epoch=PO.EPOCH, partial_blocks=M % 64 != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ou", "cha"])
def test_units_of_the_one_launch_kernel_with_a_small_net(kind, monkeypatch):
    """OU's five statistics per wave through k_paths_fb's units, bit for bit (the 4 x 128 nets of the test
    above reach k_paths_fb with Cha only); _units() shows that the one-launch kernel ran them."""
    for M in (128, 100):
        _compare(_small_generator(kind, 100, M, 3), True, True, M, 3, monkeypatch, (L.DPI_BOTH,))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cha", "ou"])
def test_ten_calls_on_one_workspace_reuse_the_join_words_and_the_rows(kind, monkeypatch):
    """Join words, extra rows, park rows and tickets are reused from call to call, across policies and
    whole-block calls: every call returns the first call's bits (a stale join word or row would not)."""
    net = "ELU" if kind == "cha" else "Tanh"  # OU 4 x 128 ELU has no units
    gen = PO._generator(kind, net, False, 100, 100, 3)
    tx, _ = gen.sample_t_and_x(N, point_base=PB)
    ws = gen.point_baseline(tx)
    plan = [POLICIES[0], ("100000", "0", "1"), ("3", "1", "2"), POLICIES[0], ("100000", "1", "1"), ("1", "0", "2"),
            ("3", "0", "1"), ("100000", "0", "2"), POLICIES[0], ("100000", "1", "2")]
    first = None
    for call, policy in enumerate(plan):
        _set(monkeypatch, policy, ("0", "4")[call % 2])
        y, mom = gen.label_moments_finalize(tx, PB, 100, L.DPI_BOTH, ws)
        assert _units() == _expected_units(policy, L.DPI_BOTH, 2 * N, 0), (call, policy)
        got = (y, mom) + PO._sample(gen, N, PB, L.DPI_BOTH)
        assert _units() == _expected_units(policy, L.DPI_BOTH, 2 * N, N if kind == "cha" else 0), (call, policy)
        torch.cuda.synchronize()
        first = got if first is None else first
        for g, w in zip(got, first):
            assert torch.equal(g, w), (call, policy)
    assert torch.equal(first[0], first[3])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["0", "1"])
@pytest.mark.parametrize("case", [("cha", 100, 3, 128, "mlp128x4-split"), ("ou", 100, 3, 128, "mlp64x2-split")],
                         ids=["cha", "ou"])
def test_all_blocks_split_against_the_fp64_oracle(case, order, monkeypatch):
    """The project's bar (tests/test_gpu_parity.py): rel-L2 < 1e-4 on the value column and on the gradient
    block, for k_paths and k_paths_fb, with every block of the call run as two units."""
    gen, tx, ref = PO._oracle(case)
    _set(monkeypatch, ("100000", order, "1"))
    y_paths = gen.generate_with_gradients(tx, point_base=0)
    assert _units() == (2 * N, 4 * N, 1)
    tx_fb, y_fb = gen.sample_generate(N, 0)
    assert _units() == (2 * N, 5 * N, 1)  # both cases' nets have a k_paths_fb instance
    torch.cuda.synchronize()
    assert torch.equal(tx_fb, tx)
    for y in (y_paths, y_fb):
        parts = C.O.rel_l2_parts(y.cpu().numpy().astype(np.float64), ref)
        print(case, order, parts)
        assert parts["value"] < 1e-4 and parts["grad"] < 1e-4, parts


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [None, ("100000", "1", "1"), ("3", "0", "2"), ("100000", "1", "2")],
                         ids=["default", "all-T-first", "3-T-finishes", "all-I-finishes"])
@pytest.mark.parametrize("kind", ["cha", "ou"])
def test_graph_replays_with_the_points_changed_between_them(kind, policy, monkeypatch):
    """A captured label call carries the same join sequence in every replay, and k_paths reads its points
    through a pointer: the caller refreshes them between replays.  Each replay must give the eager
    whole-block labels of the points it ran on — the join words of one replay must not be taken for the
    next one's (the finisher clears the word behind itself)."""
    net = "ELU" if kind == "cha" else "Tanh"  # OU 4 x 128 ELU has no units
    gen = PO._generator(kind, net, False, 100, 128, 3)
    _set(monkeypatch, POLICIES[0])
    points = [gen.sample_t_and_x(N, point_base=PB + 10 * k)[0] for k in range(3)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # also sizes the workspace before capture
        eager = [gen.generate_with_gradients(p, point_base=PB).clone() for p in points]
    torch.cuda.current_stream().wait_stream(s)
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[1], eager[2])
    if policy is None:
        for k in ("DPI_TAIL", "DPI_TAIL_ORDER", "DPI_TAIL_LAUNCHES"):
            monkeypatch.delenv(k, raising=False)
        policy = ("100000", "0", "1")  # the default rule splits all of a call this small
    else:
        _set(monkeypatch, policy)
    tx = points[0].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = gen.generate_with_gradients(tx, point_base=PB)
    assert _units() == _expected_units(policy, L.DPI_BOTH, 2 * N, 0)
    for k in (0, 1, 2, 1, 1, 0):
        tx.copy_(points[k])
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager[k]), k
    # and the replays leave the workspace (join words, tickets) fit for the next eager call
    assert torch.equal(gen.generate_with_gradients(points[2], point_base=PB), eager[2])
