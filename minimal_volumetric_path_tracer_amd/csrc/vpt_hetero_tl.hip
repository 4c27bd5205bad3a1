/*
 * vpt_hetero_tl.hip -- the kernels of estimators 10 and 11 on the trilinear field (TL = true; vpt_grid.h, vpt_hetero.h):
 * vpt_hetero.hip compiled a second time with VPT_HETERO_TL = 1, which instantiates every kernel of that file with
 * TL = true and exports its launches as vpt_int_hetero_unit_tl.  A translation unit of its own, as vpt_hetero.hip is
 * beside vpt_kernels.hip: the nearest-lookup kernels' code object stays what it was, and this one can take compile
 * flags of its own.
 */
#define VPT_HETERO_TL 1
#include "vpt_hetero.hip"
