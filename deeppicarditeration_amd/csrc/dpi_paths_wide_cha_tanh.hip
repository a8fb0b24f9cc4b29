// k_paths instantiations for DPI_EQ_CHA with state dimensions above 128 and Tanh hidden activations.
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(wide_cha_tanh)
