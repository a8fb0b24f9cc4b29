// k_paths instantiations for DPI_EQ_OU with state dimensions above 128 (up to NXW_MAX = 256): the
// first-order labels at one workgroup per CU (a unit of its own).
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(wide_ou)
