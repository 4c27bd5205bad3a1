/*
 * vpt_grid_accum.h -- what the code objects of the grid accumulator's render kernels (vpt_grid_accum.hip, compiled once
 * per estimator family and lookup) export: one launch each.  Host declarations only; vpt_kernels.hip picks the unit
 * (vpt_int_grid_pass) as hetero_unit() picks a render's.
 */
#ifndef VPT_GRID_ACCUM_H
#define VPT_GRID_ACCUM_H

#include "vpt_hetero.h"
#include "vpt_wave_accum.h"

/* the unit's persistent-wave kernel of K.est for the pass A, enqueued on `stream` on as many workgroups as the device
 * holds, at most one per four listed tiles (the caller owns the queue word K.queue and has zeroed it in stream order) */
typedef int vpt_grid_accum_launch(int device, const vpt::KParams& K, const DevScene* S, const vpt::GridAccum& A,
                                  const vpt_hetero_args& a, void* stream);

vpt_grid_accum_launch vpt_int_grid_accum_hetero, vpt_int_grid_accum_hetero_tl;        /* estimators 10 and 11 */
vpt_grid_accum_launch vpt_int_grid_accum_hetero_em, vpt_int_grid_accum_hetero_em_tl;  /* with the emission grid */
vpt_grid_accum_launch vpt_int_grid_accum_eqa, vpt_int_grid_accum_eqa_tl;              /* estimator 12 */
vpt_grid_accum_launch vpt_int_grid_accum_mis, vpt_int_grid_accum_mis_tl;              /* 13 */
vpt_grid_accum_launch vpt_int_grid_accum_chroma, vpt_int_grid_accum_chroma_tl;        /* 14 */
vpt_grid_accum_launch vpt_int_grid_accum_residual, vpt_int_grid_accum_residual_tl;    /* 15 */
vpt_grid_accum_launch vpt_int_grid_accum_spectral, vpt_int_grid_accum_spectral_tl;    /* 16 */

#endif
