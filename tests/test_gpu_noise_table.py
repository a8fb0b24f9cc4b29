"""The per-wave Philox table of the first-order rollouts (csrc/dpi_rng.h NOISE_TABLE; overlaid on the
weight ring, csrc/dpi_device.h paths_body) on the GPU, at the shapes of tests/noise_table_cases.py:
chunks of 64 steps (K = 1 .. 130), one to all waves rolling out (nx = 4, 100, 128), the ring used by
LDS-DMA / staged fp32 chunks around the rollouts, no ring use (ZeroSolution), OU, dead lanes.

1. Against the fp64 oracle (O.labels_grad on the same counters) with the bound tests/test_gpu_parity.py
   uses for this quantity: rel-L2 < 1e-4 on the value column and on the gradient block (expected
   ~1e-7; one wrong table word changes four normals of every path and misses by orders of magnitude),
   for sample_with_gradients (k_paths_fb) and generate_with_gradients (k_paths).
2. Bitwise against the plain form: tests/golden/noise_table/plain_form.npz holds the labels of the
   ZeroSolution cases and of the K = 65 / K = 130 network cases as the plain-form library
   (-DDPI_NOISE_TABLE_FO=0, tools/build_variant.py) computed them on an MI355X; the product's labels
   must equal them in every bit (np.array_equal on the uint32 view).  The fixture pins today's
   labels: a later, intended change of the label arithmetic regenerates it with
   tools/record_noise_table_golden.py."""
import functools
from pathlib import Path

import numpy as np
import pytest

import noise_table_cases as C

pytestmark = pytest.mark.gpu
TOL = 1e-4


@functools.lru_cache(maxsize=None)
def _labels(case):
    import deeppicarditeration_amd._lib as L
    L.load()  # fail loudly if the HIP library is missing
    return C.run(case)


@functools.lru_cache(maxsize=None)
def _reference(case):
    # the draws do not depend on the GEMM mode: the two modes of a net share a reference
    shared = case.replace("-f32", "-split")
    return C.reference(shared, _labels(shared)["tx"])


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("case", list(C.CASES))
def test_table_form_vs_oracle(case, entry):
    y, ref = _labels(case)[entry], _reference(case)
    if case.endswith("-f32"):  # the same points as the split run's reference
        assert np.array_equal(_labels(case)["tx"], _labels(case.replace("-f32", "-split"))["tx"])
    assert y.shape == ref.shape and np.isfinite(y).all()
    parts = C.O.rel_l2_parts(y.astype(np.float64), ref)
    print(case, entry, parts)
    assert parts["value"] < TOL and parts["grad"] < TOL, parts


@pytest.fixture(scope="module")
def golden():
    return np.load(Path(__file__).resolve().parent / "golden" / C.GOLDEN)


@pytest.mark.parametrize("case", C.PINNED)
def test_table_form_bitwise_equals_plain_form(case, golden):
    got = _labels(case)
    for what in ("tx",) + C.ENTRIES:
        want = golden[f"{case}/{what}"]
        assert got[what].dtype == np.float32 and want.dtype == np.float32 and got[what].shape == want.shape
        assert np.array_equal(got[what].view(np.uint32), want.view(np.uint32)), (case, what)
