// The head form of the general MLP family (dpi_general.h NetGenHead), row head_cha_128 of DPI_UNITS.
#include "dpi_dispatch.h"

DPI_UNIT_DEFINE(head_cha_128)
