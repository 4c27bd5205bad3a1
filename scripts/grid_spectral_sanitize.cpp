/* The host side of csrc/vpt_grid_spectral.h under -fsanitize=address,undefined: a stand-alone program that runs what the
 * host probe runs (vpt_grid_spectral_probe_host: vpt_grid_spectral_one, both walkers; nearest and trilinear, blocks 0, 1, 2,
 * 8; a grey medium, the coloured one, a coloured albedo on a grey extinction and one with a channel 64 times as dense) on
 * ray sets read from a file and on degenerate rays of its own (no length, a negative and a NaN surface distance, a zero
 * and a NaN direction, origins on the box's faces and corners, a ray in a voxel plane), with the voxels and the majorant
 * grid in heap arrays of their exact size, with the throughput (1, 1, 1), one with a channel at zero and one that carries
 * nothing.  It checks on every ray that the weights are finite and >= 0, that with beta = 1 they sum to 3 within 2^-40 and
 * that the transmittance vector is in [0, 1].  CPU only.
 *   python scripts/grid_mis_sanitize.py --dir DIR        writes tau.bin, sparse.bin, one.bin and ks.bin (and runs its own program)
 *   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I minimal_volumetric_path_tracer_amd/csrc scripts/grid_spectral_sanitize.cpp -o DIR/grid_spectral_sanitize
 *   for f in tau sparse one ks; do DIR/grid_spectral_sanitize DIR/$f.bin || exit 1; done
 * file: int32 nx, ny, nz, n; double lo[3], hi[3], sigma_t; float rho[nx ny nz]; double rays[n][6], tmax[n]; uint64 states[n] */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vpt_grid_spectral.h"

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
    int n = hdr[3];
    std::vector<float> rho((size_t)dims[0] * dims[1] * dims[2]);
    std::vector<double> rays((size_t)n * 6), tmax(n);
    std::vector<uint64_t> st(n);
    if (!rd(f, rho.data(), rho.size()) || !rd(f, rays.data(), rays.size()) || !rd(f, tmax.data(), n) || !rd(f, st.data(), n)) return 2;
    fclose(f);
    if (vpt_grid_bad(dims, box, box + 3, rho.data()) || n < 1) return 3;
    const double *lo = box, *hi = box + 3, s = box[6];
    /* the degenerate rays */
    const double mid[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
    const double nan = std::nan(""), len = hi[0] - lo[0];
    const double extra[][7] = {
        {mid[0], mid[1], mid[2], 1, 0, 0, 0.0},       {mid[0], mid[1], mid[2], 1, 0, 0, -1.0},
        {mid[0], mid[1], mid[2], 1, 0, 0, nan},       {mid[0], mid[1], mid[2], 0, 0, 0, 50 * len},
        {mid[0], mid[1], mid[2], nan, 0, 0, 1e30},    {lo[0], mid[1], mid[2], 1, 0, 0, 1e30},
        {hi[0], mid[1], mid[2], -1, 0, 0, 1e30},      {hi[0], mid[1], mid[2], 1, 0, 0, 1e30},
        {lo[0], lo[1], lo[2], 1, 0, 0, 1e30},         {hi[0], hi[1], hi[2], -1, 0, 0, 1e30},
        {lo[0] - len, lo[1] + (hi[1] - lo[1]) / dims[1], mid[2], 1, 0, 0, 1e30},
        {lo[0] - len, mid[1], mid[2], 1, 0, 0, len},  {mid[0], mid[1], mid[2], 0, 0, 1, 1e300},
    };
    for (const auto& e : extra) {
        rays.insert(rays.end(), e, e + 6);
        tmax.push_back(e[6]);
        st.push_back(0x1234ABCD330Eull + (uint64_t)n);
        n += 1;
    }
    /* {sa[3], ss[3]} per unit density */
    const double media[4][6] = {{0.25 * s, 0.25 * s, 0.25 * s, 0.75 * s, 0.75 * s, 0.75 * s},
                                {0.125 * s, 0.25 * s, 0.5 * s, 1.5 * s, 0.75 * s, 0.375 * s},
                                {0.75 * s, 0.5 * s, 0.25 * s, 0.25 * s, 0.5 * s, 0.75 * s},
                                {64.0 * s, s, 0.25 * s, 0.5 * s, 0.5 * s, 0.5 * s}};
    const double betas[3][3] = {{1.0, 1.0, 1.0}, {1.0, -0.25, 0.0}, {0.0, 0.0, 0.0}};
    double sum = 0.0, wmax = 0.0;
    unsigned long long steps = 0, counts[3] = {0, 0, 0}, bad = 0;
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
            for (const auto& md : media) {
                const double *sa = md, *ss = md + 3;
                const double stk[3] = {sa[0] + ss[0], sa[1] + ss[1], sa[2] + ss[2]};
                const vpt_spectral_consts kc = vpt_grid_spectral_consts(ss, stk);
                for (int b = 0; b < 3; ++b)
                    for (int i = 0; i < n; ++i) {
                        const double *o = &rays[6 * (size_t)i], *d = o + 3;
                        double tc, w[3], T[3];
                        uint32_t ns = 0, nr = 0;
                        uint64_t Xt = 0, Xr = 0;
                        vpt_grid_spectral_one(&G, interp, block != 0, &kc, betas[b], o, d, tmax[i], st[i] & 0xFFFFFFFFFFFFull, &tc, w,
                                              &ns, &Xt, T, &nr, &Xr);
                        steps += ns + nr;
                        counts[tc != tc ? 2 : (tc >= 0 ? 1 : 0)] += 1;
                        if (b == 0 && tc == -1.0 && !(fabs((w[0] + w[1]) + w[2] - 3.0) <= 3.0 * 0x1p-40)) bad += 1;
                        for (int k = 0; k < 3; ++k) {
                            if (!(w[k] >= 0.0 && w[k] - w[k] == 0.0)) bad += 1;
                            if (b == 0 && !(w[k] <= 3.0 * (1 + 0x1p-40))) bad += 1;
                            if (!(T[k] >= 0.0 && T[k] <= 1.0)) bad += 1;
                            if (w[k] > wmax) wmax = w[k];
                            sum += w[k] + T[k];
                        }
                    }
            }
        }
    printf("%s: %d rays, checksum %.17g, %llu steps; none / collision / cap %llu / %llu / %llu; largest weight %.6f; "
           "%llu values out of bounds\n", argv[1], n, sum, steps, counts[0], counts[1], counts[2], wmax, bad);
    return bad ? 1 : 0;
}
