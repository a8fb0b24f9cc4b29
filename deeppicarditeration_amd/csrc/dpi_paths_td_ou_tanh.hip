// k_paths TD-estimator instantiations for DPI_EQ_OU networks with Tanh hidden activations.
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(td_ou_tanh)
