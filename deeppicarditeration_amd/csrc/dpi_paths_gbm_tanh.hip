// k_paths instantiations for DPI_EQ_GBM networks with Tanh hidden activations (torch.nn.Tanh, the
// reference's default NETWORK.ACTIVATIONS, picard/config.py:61); the TD estimators in
// dpi_paths_td_gbm_tanh.hip.
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(gbm_tanh)
