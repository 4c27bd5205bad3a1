/* The host side of residual ratio tracking (csrc/vpt_grid.h: vpt_grid_residual_lm_m and the control builders) under
 * -fsanitize=address,undefined: a stand-alone program that runs what the host probe runs (vpt_grid_residual_probe_host),
 * nearest and trilinear, at blocks 1, 2, 8 and max(n) + 1, on rays it generates itself (a 48-bit LCG; no input file), with
 * the voxels and each of the two block grids -- the majorants and the minima -- in a heap array of its exact size, so a read
 * one element past either is caught.  It checks 0 <= That <= 1 on every ray.  CPU only.
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
 *       -I minimal_volumetric_path_tracer_amd/csrc scripts/grid_residual_sanitize.cpp -o grid_residual_sanitize
 *   ./grid_residual_sanitize */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vpt_grid.h"

static uint64_t lcg = 0x1234ABCD330Eull;
static double uni()
{
    lcg = (lcg * 0x5DEECE66Dull + 0xBull) & 0xFFFFFFFFFFFFull;
    return (double)lcg / 281474976710656.0;
}

int main()
{
    const int32_t dims[3] = {19, 9, 11};  /* no dimension a multiple of 2 or 8: partial last blocks */
    const double lo[3] = {-1.0, 2.0, -3.0}, hi[3] = {5.0, 4.5, 7.0};
    const size_t nv = (size_t)dims[0] * dims[1] * dims[2];
    const int n = 20000;
    unsigned long long steps = 0, zeros = 0, nodraw = 0, analytic = 0, bad = 0;
    double sum = 0.0;
    for (int floor = 0; floor < 2; ++floor) {
        /* about half the voxels empty (floor 0) or every voxel at least 0.5 (floor 1) */
        float* rho = (float*)malloc(nv * sizeof(float));
        for (size_t k = 0; k < nv; ++k) rho[k] = (float)((uni() < 0.5 ? 0.0 : 0.2 + 2.8 * uni()) + 0.5 * floor);
        if (vpt_grid_bad(dims, lo, hi, rho)) return 3;
        std::vector<double> rays((size_t)n * 6), tmax(n);
        std::vector<uint64_t> st(n);
        for (int i = 0; i < n; ++i) {  /* from a point around the box (every third inside it) toward a point inside it */
            double a[3], b[3], len = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double ext = hi[k] - lo[k];
                a[k] = i % 3 == 0 ? lo[k] + (0.01 + 0.98 * uni()) * ext : lo[k] - 0.6 * ext + 2.2 * ext * uni();
                b[k] = lo[k] + (0.01 + 0.98 * uni()) * ext;
                len += (b[k] - a[k]) * (b[k] - a[k]);
            }
            len = sqrt(len);
            for (int k = 0; k < 3; ++k) {
                rays[6 * (size_t)i + k] = a[k];
                rays[6 * (size_t)i + 3 + k] = i % 7 == 0 && k != i % 3 ? 0.0 : (b[k] - a[k]) / len;  /* every 7th along an axis */
            }
            if (i % 7 == 0) rays[6 * (size_t)i + 3 + i % 3] = b[i % 3] >= a[i % 3] ? 1.0 : -1.0;
            tmax[i] = i % 4 == 0 ? len : (i % 11 == 0 ? 0.0 : 1e30);
            st[i] = (uint64_t)(uni() * 281474976710656.0);
        }
        for (int interp = 0; interp < 2; ++interp)
            for (int block : {1, 2, 8, 20 /* max(n) + 1: one super-voxel */}) {
                vpt_grid_view G;
                vpt_grid_view_init(&G, dims, lo, hi, rho, rho);
                G.interp = interp;
                int32_t nb[3];
                vpt_grid_majorant_counts(dims, block, nb);
                const size_t nbv = (size_t)nb[0] * nb[1] * nb[2];
                float* maj = (float*)malloc(nbv * sizeof(float));
                float* ctl = (float*)malloc(nbv * sizeof(float));
                if (interp) {
                    vpt_grid_majorant_build_tl(dims, block, rho, maj);
                    vpt_grid_control_build_tl(dims, block, rho, ctl);
                } else {
                    vpt_grid_majorant_build(dims, block, rho, maj);
                    vpt_grid_control_build(dims, block, rho, ctl);
                }
                vpt_grid_view_set_majorant(&G, block, maj);
                for (size_t k = 0; k < nbv; ++k)
                    if (!(ctl[k] <= maj[k] && ctl[k] >= 0.0f)) ++bad;
                for (double sigma_t : {0.7, 0.05})
                    for (int i = 0; i < n; ++i) {
                        const double *o = &rays[6 * (size_t)i], *d = o + 3;
                        uint64_t X = st[i] & 0xFFFFFFFFFFFFull;
                        uint32_t ns = 0;
                        double tauc = -1.0;
                        const double T = vpt_grid_residual_lm_m(&G, ctl, interp, o, d, tmax[i], sigma_t, &X, &ns, &tauc);
                        if (!(T >= 0.0 && T <= 1.0) || !(tauc >= 0.0)) {
                            if (++bad < 10) printf("ray %d (floor %d, interp %d, block %d): That %.17g tauc %.17g\n", i, floor, interp, block, T, tauc);
                        }
                        steps += ns;
                        zeros += T == 0.0;
                        nodraw += ns == 0;
                        analytic += ns == 1 && tauc > 0.0;
                        sum += T + tauc;
                    }
                free(ctl);
                free(maj);
            }
        free(rho);
    }
    printf("%d rays x 2 fields x 2 lookups x 4 blocks x 2 sigma_t: checksum %.17g, %llu draws, %llu zeros, %llu without a draw, "
           "%llu with one draw and a control depth, %llu out of range\n", n, sum, steps, zeros, nodraw, analytic, bad);
    return bad ? 1 : 0;
}
