// k_paths instantiations for DPI_EQ_GBM (first-order SDGD / exact-diagonal labels) with state
// dimensions above 128 (up to NXW_MAX = 256): W1x read from L2, a unit of its own.
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(wide_gbm)
