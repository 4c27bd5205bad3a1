/*
 * vpt_hetero_mis_tl.hip -- the kernels of estimator 13 on the trilinear field (TL = true; vpt_grid.h, vpt_hetero_mis.h):
 * vpt_hetero_mis.hip compiled a second time with VPT_HETERO_TL = 1, which instantiates every kernel of that file with
 * TL = true and exports its launches as vpt_int_hetero_mis_unit_tl, as vpt_hetero_eqa_tl.hip does for estimator 12.
 */
#define VPT_HETERO_TL 1
#include "vpt_hetero_mis.hip"
