// The terminal-enforcing head form of the general MLP family (dpi_general.h TERMA), row term_head_cha_256_tanh of DPI_UNITS.
#include "dpi_dispatch.h"

DPI_UNIT_DEFINE(term_head_cha_256_tanh)
