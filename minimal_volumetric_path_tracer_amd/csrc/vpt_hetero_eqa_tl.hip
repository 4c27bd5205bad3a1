/*
 * vpt_hetero_eqa_tl.hip -- the kernels of estimator 12 on the trilinear field (TL = true; vpt_grid.h, vpt_hetero_eqa.h):
 * vpt_hetero_eqa.hip compiled a second time with VPT_HETERO_TL = 1, which instantiates every kernel of that file with
 * TL = true and exports its launches as vpt_int_hetero_eqa_unit_tl, as vpt_hetero_tl.hip does for estimators 10 and 11.
 */
#define VPT_HETERO_TL 1
#include "vpt_hetero_eqa.hip"
