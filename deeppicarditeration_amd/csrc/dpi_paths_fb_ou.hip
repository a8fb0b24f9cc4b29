// k_paths_fb instantiations for DPI_EQ_OU (the one-launch dpi_sample_with_gradients; a unit of its own).
#include "dpi_dispatch.h"
DPI_UNIT_DEFINE(fb_ou)
