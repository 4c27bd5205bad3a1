/*
 * vpt_hetero_spectral_tl.hip -- the kernels of estimator 16 on the trilinear field (TL = true; vpt_grid.h,
 * vpt_hetero_spectral.h): vpt_hetero_spectral.hip compiled a second time with VPT_HETERO_TL = 1, which instantiates every
 * kernel of that file with TL = true and exports its launches as vpt_int_hetero_spectral_unit_tl, as
 * vpt_hetero_chroma_tl.hip does for estimator 14.
 */
#define VPT_HETERO_TL 1
#include "vpt_hetero_spectral.hip"
