/* The host side of csrc/vpt_grid.h under -fsanitize=address,undefined: a stand-alone program that runs what the host
 * probes run (vpt_grid_probe_host_ex, vpt_grid_ratio_probe_host_ex: the optical depth, the track and the ratio estimate,
 * nearest and trilinear, blocks 0, 1, 2, 8) on ray sets read from a file, with the voxels and the majorant grid in heap
 * arrays of their exact size.  CPU only.  scripts/grid_sanitize.py writes the sets, builds and runs it.
 * file: int32 nx, ny, nz, n; double lo[3], hi[3], sigma_t; float rho[nx ny nz]; double rays[n][6], tmax[n]; uint64 states[n] */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vpt_grid.h"

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
    if (vpt_grid_bad(dims, box, box + 3, rho.data())) return 3;
    double sum = 0.0;
    unsigned long long steps = 0;
    for (int interp = 0; interp < 2; ++interp)
        for (int block : {0, 1, 2, 8}) {
            vpt_grid_view G;
            vpt_grid_view_init(&G, dims, box, box + 3, rho.data(), rho.data());
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
            for (int i = 0; i < n; ++i) {
                const double *o = &rays[6 * (size_t)i], *d = o + 3;
                uint64_t X = st[i] & 0xFFFFFFFFFFFFull;
                uint32_t ns = 0;
                sum += interp ? vpt_grid_tau_tl(&G, o, d, tmax[i]) : vpt_grid_tau(&G, o, d, tmax[i]);
                const double tc = block ? vpt_grid_track_lm_m(&G, interp, o, d, tmax[i], box[6], &X, &ns)
                                        : vpt_grid_track_m(&G, interp, o, d, tmax[i], box[6], &X, &ns);
                steps += ns;
                if (tc == tc) sum += tc;
                X = st[i] & 0xFFFFFFFFFFFFull;
                sum += block ? vpt_grid_ratio_lm_m(&G, interp, o, d, tmax[i], box[6], &X, &ns)
                             : vpt_grid_ratio_m(&G, interp, o, d, tmax[i], box[6], &X, &ns);
                steps += ns;
            }
        }
    printf("%s: %d rays, checksum %.17g, %llu steps\n", argv[1], n, sum, steps);
    return 0;
}
