// k_paths instantiations for DPI_EQ_CHA networks with Tanh hidden activations (torch.nn.Tanh, the
// reference's default NETWORK.ACTIVATIONS, picard/config.py:61); the TD estimators in
// dpi_paths_td_cha_tanh.hip.
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(cha_tanh)
