// bfhip_ridge.h -- shapes shared by the kernels of bfhip_ridge.hip (bfhip_ridge_path, bfhip_ridge_rotate: include/bfhip.h).
#pragma once
#include "bfhip_common.h"

#define RG_ROWS BFHIP_RIDGE_TILE   // rows of Z per workgroup: 16 per wave
#define RG_OB 16                   // outputs per workgroup: the columns of one MFMA tile
#define RG_LC 8                    // penalties per sweep of a wave over the columns of Z (8 accumulator tiles of 16 x 16)
#define RG_LP BFHIP_RIDGE_MAX_L    // row stride of the weight table g (r, RG_LP): zero beyond L
#define RG_NS 7                    // sums a partial carries (BFHIP_LOO_SSE .. BFHIP_LOO_NUNIT)
static_assert(RG_ROWS == 64 && RG_LP % RG_LC == 0, "four waves of 16 rows; whole sweeps of the weight table");
