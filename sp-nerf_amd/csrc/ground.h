// The host check every ground-grid entry point makes of a grid's size before it launches anything.
#pragma once
#include <cstdint>

#include "common.h"

namespace spn {

// H x W cells, both positive, at most 2^32 of them (a cell index fits the kernels' arithmetic); the messages name
// the grid as "W x H", which tests/test_*_abi.py pin per export
inline int32_t check_cells(const char* who, int32_t ysize, int32_t xsize) {
    SPN_ARG(xsize > 0 && ysize > 0, "%s: grid of %d x %d cells", who, xsize, ysize);
    SPN_ARG((int64_t)xsize * ysize <= ((int64_t)1 << 32), "%s: grid of %d x %d cells is too large for one call", who, xsize, ysize);
    return SPNERF_OK;
}

}  // namespace spn
