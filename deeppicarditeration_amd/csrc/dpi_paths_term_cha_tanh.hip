// The terminal-enforcing form of the general MLP family (dpi_general.h TERMA), row term_cha_tanh of DPI_UNITS.
#include "dpi_dispatch.h"

DPI_UNIT_DEFINE(term_cha_tanh)
