"""The numpy restatement of the PISGradNet shell (tests/pis_shell_reference.py) against torch fp64 autograd — CPU
only.  It is the yardstick of tests/test_gpu_pis_shell.py, so it is itself held to torch here: stage by stage
against PISGradNet's own submodules, chained around the restated core against the whole objective on the 14
cases of tests/pis_fit_reference.py, and shown to see each term of the math through a mutant that drops it."""
import numpy as np
import pytest
import torch

import pis_fit_reference as R
import pis_shell_reference as S

PAIRS = [(k, m) for k in range(len(S.CASES)) for m in S.MODES]
PAIR_IDS = [f"{S.IDS[k]}-{m}" for k, m in PAIRS]
CAP = 5e-6  # of E_case on the GPU (tests/test_gpu_pis_shell.py): the bar there never exceeds 2e-5


@pytest.mark.parametrize("k,mode", PAIRS, ids=PAIR_IDS)
def test_stages_equal_torch_fp64(k, mode):
    """Every output of every stage to 1e-12 rel-L2 of torch fp64; an output torch gives as exact zeros (smooth_net's
    last bias gradient, the rows >= 1 of its last weight gradient) is exactly zero."""
    got, want, names = S.stage_outputs(k, mode), S.torch_stages(k, mode), S.stage_names(k)
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        assert (g is None) == (w is None), name
        if g is None:
            continue
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if not np.any(w):
            assert not np.any(g), name
        else:
            assert R.rel_l2(g, w) <= 1e-12, (name, R.rel_l2(g, w))
    depth = S.CASES[k][2]
    last_w = got[names.index(f"d smooth_net.{2 * (depth + 1)}.weight")]
    assert np.any(last_w[0]) and not np.any(last_w[1:])
    assert (mode == "grad") == (got[names.index("res_x")] is not None) == (got[names.index("r")] is not None)


@pytest.mark.parametrize("k", range(len(R.CASES)), ids=R.IDS)
def test_chain_reproduces_the_objective(k):
    """The three stages around R.core_forward / R.core_backward: the loss and every parameter gradient of the
    whole PISGradNet to 1e-12 of torch fp64 autograd; smooth_net's last bias gradient absolutely."""
    loss, grads = S.chain(k)
    want_loss, want = R.torch_fp64(k)
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
    names = R.param_names(R.CASES[k])
    assert len(grads) == len(want) == len(names)
    top = max(float(np.linalg.norm(w)) for w in want)
    for name, g, w in zip(names, grads, want):
        assert g.shape == w.shape, name
        if np.any(w):
            assert R.rel_l2(g, w) <= 1e-12, (name, R.rel_l2(g, w))
        else:
            assert float(np.abs(g).max()) <= 1e-12 * top, name


# the output a mutant concerns: the stage output whose formula it changes, or, for a term of the reverse pass, the
# parameter tensors that term feeds (a name prefix)
CONCERNS = {"no_zero_point": "s", "no_cos_half": "timestep_phase", "no_c_res_x": "res_x", "no_g_sbar": "sbar",
            "e_unscaled": "e", "zero_seed_sign": "smooth_net."}


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_mutants_are_seen(mutant):
    """Each mutant moves the output it concerns by >= 1e-3 rel-L2 in fp64 (the largest over the tensors of a
    prefix) on every stage case and mode that reaches it — the table the GPU test runs; the value kind reaches
    neither res_x nor the gradient-loss part of sbar, and is left bit for bit alone by those two.  (Through the
    chain on R.CASES the gradient-loss part of sbar is smaller where res ~ nx dominates sbar: dropping it moves
    sbar by 6.1e-4 at B100-nx100-T0.5, which is why the gate stands on the stages' own draws.)"""
    assert set(CONCERNS) == set(S.MUTANTS)
    for k, mode in PAIRS:
        clean, got, names = S.stage_outputs(k, mode), S.stage_outputs(k, mode, mutant=mutant), S.stage_names(k)
        if mode == "value" and mutant in S.VALUE_BLIND:
            assert all((g is None and c is None) or np.array_equal(g, c) for g, c in zip(got, clean))
            continue
        what = CONCERNS[mutant]
        moved = max(R.rel_l2(g, c) for n, g, c in zip(names, got, clean)
                    if (n == what or (what.endswith(".") and n.startswith("d " + what)) or n == "d " + what)
                    and np.any(c))
        assert moved >= 1e-3, (mutant, S.IDS[k], mode, moved)


@pytest.mark.parametrize("k,mode", PAIRS, ids=PAIR_IDS)
def test_fp32_evaluations_stay_under_the_cap(k, mode):
    """The cap the GPU test puts on E_case — the largest error of any output of the case over two fp32
    evaluations of the reference — holds on the CPU for seeds 0 - 2: torch fp32 and the restatement in fp32."""
    for seed in range(3):
        want = S.stage_outputs(k, mode, seed=seed)
        pool = (S.stage_errors(S.torch_stages(k, mode, torch.float32, seed=seed), want)
                + S.stage_errors(S.stage_outputs(k, mode, np.float32, seed=seed), want))
        worst = max((e, n) for e, n in zip(pool, S.stage_names(k) * 2) if e is not None)
        print(f"PIS_SHELL_CAP {S.IDS[k]} {mode} seed {seed} E_case {worst[0]:.3e} ({worst[1]})")
        assert worst[0] <= CAP, (seed, worst)
