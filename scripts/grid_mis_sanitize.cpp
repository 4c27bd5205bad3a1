/* The host side of csrc/vpt_grid_mis.h under -fsanitize=address,undefined: a stand-alone program that runs what the
 * host probe runs (vpt_grid_mis_probe_host: vpt_grid_mis_one, nearest and trilinear, blocks 0, 1, 2, 8, the track fractions
 * 0, 0.25, 0.5, 1, a light inside the box, one outside it and one on the first ray's line) on ray sets read from a file,
 * with the voxels and the majorant grid in heap arrays of their exact size.  CPU only.  scripts/grid_mis_sanitize.py
 * writes the sets (the files of scripts/grid_sanitize.py), builds and runs it.
 * file: int32 nx, ny, nz, n; double lo[3], hi[3], sigma_t; float rho[nx ny nz]; double rays[n][6], tmax[n]; uint64 states[n] */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vpt_grid_mis.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n)
{
    return fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4];
    double box[7];
    if (!rd(f, hdr, 4) || !rd(f, box, 7)) return 2;
    const int32_t dims[3] = {hdr[0], hdr[1], hdr[2]};
    const int n = hdr[3];
    std::vector<float> rho((size_t)dims[0] * dims[1] * dims[2]);
    std::vector<double> rays((size_t)n * 6), tmax(n);
    std::vector<uint64_t> st(n);
    if (!rd(f, rho.data(), rho.size()) || !rd(f, rays.data(), rays.size()) || !rd(f, tmax.data(), n) || !rd(f, st.data(), n)) return 2;
    fclose(f);
    if (vpt_grid_bad(dims, box, box + 3, rho.data()) || n < 1) return 3;
    const double *lo = box, *hi = box + 3;
    const double lights[3][3] = {
        {lo[0] + 0.4 * (hi[0] - lo[0]), lo[1] + 0.45 * (hi[1] - lo[1]), lo[2] + 0.55 * (hi[2] - lo[2])},
        {hi[0] + 2.5, hi[1] + 1.5, lo[2] - 3.0},
        {rays[0] + 0.5 * rays[3], rays[1] + 0.5 * rays[4], rays[2] + 0.5 * rays[5]}};  /* D == 0 for ray 0: 0 / 0 */
    double sum = 0.0;
    unsigned long long steps = 0, counts[4] = {0, 0, 0, 0};
    for (int interp = 0; interp < 2; ++interp)
        for (int block : {0, 1, 2, 8}) {
            vpt_grid_view G;
            vpt_grid_view_init(&G, dims, lo, hi, rho.data(), rho.data());
            G.interp = interp;
            std::vector<float> maj;
            if (block) {
                int32_t nb[3];
                vpt_grid_majorant_counts(dims, block, nb);
                maj.resize((size_t)nb[0] * nb[1] * nb[2]);
                if (interp) vpt_grid_majorant_build_tl(dims, block, rho.data(), maj.data());
                else vpt_grid_majorant_build(dims, block, rho.data(), maj.data());
                vpt_grid_view_set_majorant(&G, block, maj.data());
            }
            for (double q : {0.0, 0.25, 0.5, 1.0})
                for (const auto& lp : lights)
                    for (int i = 0; i < n; ++i) {
                        const double *o = &rays[6 * (size_t)i], *d = o + 3;
                        uint64_t X = st[i] & 0xFFFFFFFFFFFFull;
                        double ps, ds, pf, pe, tr, rt;
                        int sg = 0;
                        uint32_t ns = 0;
                        vpt_grid_mis_one(&G, interp, block != 0, box[6], q, o, d, tmax[i], lp, &X, &ps, &sg, &ds, &pf, &pe, &tr,
                                         &rt, &ns);
                        steps += ns;
                        counts[2 * sg + (ds == -1.0 ? 0 : 1)] += 1;
                        sum += ps + tr + rt;
                        if (pf == pf && pf < 1e300) sum += pf;
                    }
        }
    printf("%s: %d rays, checksum %.17g, %llu steps; equi-angular surface / medium %llu / %llu, track %llu / %llu\n", argv[1],
           n, sum, steps, counts[0], counts[1], counts[2], counts[3]);
    return 0;
}
