// k_baseline / k_paths instantiations for DPI_EQ_CHA (one translation unit per equation family).
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(cha)
