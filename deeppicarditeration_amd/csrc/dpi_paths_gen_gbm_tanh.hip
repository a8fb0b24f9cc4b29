// The general MLP family on GBM (dpi_general_gbm.h), row gen_gbm_tanh of DPI_UNITS.
#include "dpi_dispatch.h"

DPI_UNIT_DEFINE(gen_gbm_tanh)
