// k_baseline / k_paths instantiations for DPI_EQ_GBM (one translation unit per equation family).
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(gbm)
