"""Monte-Carlo sample counts that are no multiple of the 64-path block, host side (no GPU):
the reference-made fixtures under tests/golden/partial/ pin the oracle at such counts, and the
relaxed argument rules of the C ABI and of ShardedLabeler.shard hold before any device work."""
import ctypes

import numpy as np
import pytest

from golden_util import GOLDEN, delta_t, load, m_terminal, oracle_equation, oracle_net, t_factors
from oracle import dpi_oracle as O

PARTIAL = ["cha_mlp16_M100_K2", "cha_mlp16_M1_K2", "ou_pis32_M65_K2", "gbm_mlp32x3_M100_MT37_K2",
           "gbm_hess_mlp32x3_M100_K2"]
TOL = 1e-12  # both sides are fp64 and differ in summation order only


def test_the_partial_fixtures_are_these_five():
    assert sorted(p.stem for p in (GOLDEN / "partial").glob("*.npz")) == sorted(PARTIAL)
    counts = {c: (m_terminal(load(f"partial/{c}")), int(load(f"partial/{c}")["M"])) for c in PARTIAL}
    assert all(mt % 64 or m % 64 for mt, m in counts.values())
    assert counts["gbm_mlp32x3_M100_MT37_K2"] == (37, 100) and counts["cha_mlp16_M1_K2"] == (1, 1)


@pytest.mark.parametrize("case", PARTIAL)
def test_oracle_matches_reference_at_partial_counts(case):
    f = load(f"partial/{case}")
    eq = oracle_equation(f)
    net = oracle_net(f, eq)
    n, nx, M, K = int(f["n"]), eq.nx, int(f["M"]), int(f["K"])
    seed, epoch, pb = int(f["seed"]), int(f["epoch"]), int(f["point_base"])
    if bool(f["hessians"]):
        tx = O.sample_points(eq, n, seed, epoch, pb)
        y = O.labels_grad_hess(eq, net, tx, M, K, seed, epoch, pb, MT=m_terminal(f))
        blocks = (("value", slice(0, 1)), ("grad", slice(1, 1 + nx)), ("hess", slice(1 + nx, None)))
    else:
        tx, y = O.sample_with_gradients(eq, net, n, M, K, seed, epoch, pb, int(f["v"]), delta_t=delta_t(f),
                                        t_factors=t_factors(f), MT=m_terminal(f))
        blocks = (("value", slice(0, 1)), ("grad", slice(1, None)))
    np.testing.assert_allclose(tx, f["tx"], rtol=0, atol=1e-13)
    assert y.shape == f["y"].shape
    for name, sl in blocks:
        r = O.rel_l2(y[:, sl], f["y"][:, sl])
        print(case, name, r)
        assert r <= TOL, (name, r)


def test_shard_takes_any_count_on_one_rank():
    from deeppicarditeration_amd.sharding import ShardedLabeler
    assert ShardedLabeler(None, 0, 1).shard(100) == (0, 100)
    assert ShardedLabeler(None, 0, 1).shard(1) == (0, 1)
    assert ShardedLabeler(None, 0, 1).shard(4096) == (0, 4096)
    with pytest.raises(ValueError):
        ShardedLabeler(None, 0, 2).shard(100)


def test_abi_version_is_8():
    from deeppicarditeration_amd import _lib
    assert _lib.DPI_ABI_VERSION == 8 and _lib.load().dpi_abi_version() == 8


def test_label_call_range_rules_without_gpu():
    """m_begin a multiple of 64; m_end a multiple of 64 or M.  Validation runs before any device
    work: with a workspace of 0 bytes a legal range gets as far as DPI_ERR_WORKSPACE."""
    from deeppicarditeration_amd import _lib
    lib = _lib.load()
    h, n = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.dpi_problem_create_cha(100, 1.0, 5.0, 1.0, h) == 0
    assert lib.dpi_net_create_zero(n) == 0
    try:
        p16 = ctypes.c_void_p(16)
        # the empty batch at a ragged M
        assert lib.dpi_generate_with_gradients(h, n, None, 0, 100, 50, 1, 0, 0, 3, 1e9, None, None, None, 0,
                                               None) == 0
        assert lib.dpi_label_moments(h, n, None, 0, 100, 50, 1, 0, 0, 0, 100, 3, None, None, 0, None) == 0
        assert lib.dpi_generate_with_gradients_and_hessians(h, n, None, 0, 100, 50, 1, 0, 0, 1e9, None, None, 0,
                                                            None) == 0
        assert lib.dpi_workspace_bytes(h, n, 16, 100) == lib.dpi_workspace_bytes(h, n, 16, 128)
        assert lib.dpi_workspace_bytes(h, n, 16, 1) == lib.dpi_workspace_bytes(h, n, 16, 64)

        def moments(M, m0, m1, ws_bytes=0):
            return lib.dpi_label_moments(h, n, p16, 4, M, 50, 1, 0, 0, m0, m1, 3, p16, p16, ws_bytes, None)

        # a range that ends inside a block before M is still refused
        assert moments(4096, 0, 100, 1 << 30) == _lib.DPI_ERR_ARG and "multiple of 64" in _lib.last_error()
        assert moments(200, 64, 100) == _lib.DPI_ERR_ARG and "multiple of 64" in _lib.last_error()
        # m_begin stays a multiple of 64; the range stays within [0, M] and non-empty
        assert moments(100, 32, 100) == _lib.DPI_ERR_ARG
        assert moments(100, 0, 101) == _lib.DPI_ERR_ARG
        assert moments(100, 64, 64) == _lib.DPI_ERR_ARG
        assert moments(0, 0, 0) == _lib.DPI_ERR_ARG
        # legal ranges pass validation and stop at the workspace check
        for M, m0, m1 in ((100, 0, 100), (100, 64, 100), (100, 0, 64), (1, 0, 1), (65, 64, 65)):
            assert moments(M, m0, m1) == _lib.DPI_ERR_WORKSPACE, (M, m0, m1, _lib.last_error())
        # the per-call cap counts launched blocks
        assert moments(65536 + 37, 0, 65536 + 37, 1 << 40) == _lib.DPI_ERR_ARG
        assert "DPI_PATHS_PER_CALL_MAX" in _lib.last_error()
        assert moments(65536 + 37, 65536, 65536 + 37) == _lib.DPI_ERR_WORKSPACE
        assert lib.dpi_label_prepare(h, n, p16, 4, 100, 50, 1, 0, 0, 0, 100, 3, p16, 0, None) == _lib.DPI_ERR_WORKSPACE
        # Hessian labels: 1 <= M <= 65536
        hess = lib.dpi_generate_with_gradients_and_hessians
        assert hess(h, n, p16, 4, 0, 50, 1, 0, 0, 1e9, p16, p16, 0, None) == _lib.DPI_ERR_ARG
        assert hess(h, n, p16, 4, 65537, 50, 1, 0, 0, 1e9, p16, p16, 0, None) == _lib.DPI_ERR_ARG
        assert hess(h, n, p16, 4, 100, 50, 1, 0, 0, 1e9, p16, p16, 0, None) == _lib.DPI_ERR_UNSUPPORTED  # Cha: named
    finally:
        assert lib.dpi_net_destroy(n) == 0 and lib.dpi_problem_destroy(h) == 0


def test_binding_class_takes_any_count_with_or_without_a_base():
    """The class hip_online_data_generator instantiates opts in by a class default, not by a keyword
    it would have to add to the data module's `kws`; generator_class itself is unchanged."""
    from deeppicarditeration_amd.data import OnlineDataGenerator
    from deeppicarditeration_amd.picard_binding import _any_count, generator_class

    class Base:
        pass

    assert OnlineDataGenerator.partial_blocks_default is False
    assert generator_class(None) is OnlineDataGenerator
    derived = generator_class(Base)
    assert derived.partial_blocks_default is True and _any_count(derived) is derived
    sub = _any_count(OnlineDataGenerator)
    assert sub is not OnlineDataGenerator and issubclass(sub, OnlineDataGenerator)
    assert sub.partial_blocks_default is True and _any_count(OnlineDataGenerator) is sub
