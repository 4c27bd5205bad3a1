/*
 * vpt_hetero_chroma_tl.hip -- the kernels of estimator 14 on the trilinear field (TL = true; vpt_grid.h,
 * vpt_hetero_chroma.h): vpt_hetero_chroma.hip compiled a second time with VPT_HETERO_TL = 1, which instantiates every
 * kernel of that file with TL = true and exports its launches as vpt_int_hetero_chroma_unit_tl, as vpt_hetero_mis_tl.hip
 * does for estimator 13.
 */
#define VPT_HETERO_TL 1
#include "vpt_hetero_chroma.hip"
