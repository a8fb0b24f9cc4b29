"""Host-only surface of the general MLP family (include/dpi.h dpi_pair_family, dpi_general_slots):
declared to ctypes, and null handles are argument errors before any device work."""
import ctypes

from deeppicarditeration_amd import _lib


def test_signatures_have_the_family_queries():
    assert _lib.SIGNATURES["dpi_pair_family"] == (_lib.c_int, [_lib.c_void_p, _lib.c_void_p, _lib.c_int,
                                                               _lib.P(_lib.c_int)])
    assert _lib.SIGNATURES["dpi_general_slots"] == (_lib.c_int, [_lib.c_void_p, _lib.P(_lib.c_int)])
    assert (_lib.DPI_FAMILY_SPECIALISED, _lib.DPI_FAMILY_GENERAL) == (0, 1)


def test_null_handles_are_argument_errors_without_a_gpu():
    lib = _lib.load()
    fam, slots = _lib.c_int(-7), _lib.c_int(-7)
    assert lib.dpi_pair_family(None, None, 0, ctypes.byref(fam)) == _lib.DPI_ERR_ARG
    assert "pair_family" in _lib.last_error() and fam.value == -7
    assert lib.dpi_general_slots(None, ctypes.byref(slots)) == _lib.DPI_ERR_ARG and slots.value == -7
    p, n = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.dpi_problem_create_cha(7, 1.0, 5.0, 1.0, p) == 0 and lib.dpi_net_create_zero(n) == 0
    assert lib.dpi_pair_family(p, None, 0, ctypes.byref(fam)) == _lib.DPI_ERR_ARG
    assert lib.dpi_pair_family(None, n, 0, ctypes.byref(fam)) == _lib.DPI_ERR_ARG
    assert lib.dpi_pair_family(p, n, 0, None) == _lib.DPI_ERR_ARG
    assert lib.dpi_general_slots(n, None) == _lib.DPI_ERR_ARG
    # a zero net is served by the specialised kernels and has no stash
    assert lib.dpi_pair_family(p, n, 0, ctypes.byref(fam)) == 0 and fam.value == _lib.DPI_FAMILY_SPECIALISED
    assert lib.dpi_general_slots(n, ctypes.byref(slots)) == 0 and slots.value == 0
    assert lib.dpi_net_destroy(n) == 0 and lib.dpi_problem_destroy(p) == 0
