/*
 * vpt_hetero_residual_tl.hip -- the kernels of estimator 15 on the trilinear field (TL = true; vpt_grid.h,
 * vpt_hetero_residual.h): vpt_hetero_residual.hip compiled a second time with VPT_HETERO_TL = 1, which instantiates every
 * kernel of that file with TL = true and exports its launches as vpt_int_hetero_residual_unit_tl, as vpt_hetero_eqa_tl.hip
 * does for estimator 12.
 */
#define VPT_HETERO_TL 1
#include "vpt_hetero_residual.hip"
