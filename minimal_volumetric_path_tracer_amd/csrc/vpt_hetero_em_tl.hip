/*
 * vpt_hetero_em_tl.hip -- vpt_hetero_em.hip's kernels on the trilinear field (EM = true, TL = true): vpt_hetero.hip compiled
 * with both switches, exporting vpt_int_hetero_unit_em_tl.
 */
#define VPT_HETERO_EM 1
#define VPT_HETERO_TL 1
#include "vpt_hetero.hip"
