// The head form of the general MLP family (dpi_general.h NetGenHead), row head_ou_256_tanh of DPI_UNITS.
#include "dpi_dispatch.h"

DPI_UNIT_DEFINE(head_ou_256_tanh)
