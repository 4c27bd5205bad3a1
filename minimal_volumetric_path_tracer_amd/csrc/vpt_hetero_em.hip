/*
 * vpt_hetero_em.hip -- the kernels of estimators 10 and 11 with an emission grid (EM = true; vpt_grid.h, vpt_hetero.h):
 * vpt_hetero.hip compiled with VPT_HETERO_EM = 1, which instantiates its render and per-sample kernels with EM = true and
 * the emitting track's probe, and exports the launches as vpt_int_hetero_unit_em.  A code object of its own, like
 * vpt_hetero_tl.hip: the kernels without emission stay what they were.
 */
#define VPT_HETERO_EM 1
#include "vpt_hetero.hip"
