// The general MLP family (dpi_general.h), row gen_ou of DPI_UNITS.
#include "dpi_dispatch.h"

DPI_UNIT_DEFINE(gen_ou)
