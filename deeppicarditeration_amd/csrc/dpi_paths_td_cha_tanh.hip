// k_paths TD-estimator instantiations for DPI_EQ_CHA networks with Tanh hidden activations.
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(td_cha_tanh)
