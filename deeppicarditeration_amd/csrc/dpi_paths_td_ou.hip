// k_paths TD-estimator instantiations for DPI_EQ_OU (ESTIMATE_DELTA_T > 0; a unit of their own).
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(td_ou)
