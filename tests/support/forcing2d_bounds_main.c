/* tests/support/forcing2d_bounds_main.c -- TEST INFRASTRUCTURE: a stand-alone program that runs icar_amd/csrc/forcing2d_cell.h on heap
 * allocations of exactly the reference's extents, to be built with the address and undefined-behaviour sanitizers
 * (tests/test_forcing2d_oracle.py).  Without an argument it runs the smallest grids (a 3 x 3 tile from a 2 x 2 forcing grid, every corner
 * of the forcing grid named by some cell); with a file name it reads a case written by the test: four INTEGERs nx, ny, nx_f, ny_f, then
 * geolut x, y (4, nx, ny) INTEGER, w (4, nx, ny) REAL, the forcing array (nx_f, ny_f) REAL -- and with a second one it writes the
 * interpolated field there.  Prints one line and returns 0; a sanitizer finding ends it with its own report and status. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../icar_amd/csrc/forcing2d_cell.h"

static void *take(size_t bytes)
{
    void *p = malloc(bytes);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    return p;
}

static void get(void *p, size_t bytes, FILE *f)
{
    if (fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short case file\n"); exit(2); }
}

int main(int argc, char **argv)
{
    int dims[4] = {3, 3, 2, 2};
    FILE *f = NULL;
    if (argc > 1) {
        f = fopen(argv[1], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
        get(dims, sizeof dims, f);
    }
    const int nx = dims[0], ny = dims[1], nx_f = dims[2], ny_f = dims[3];
    if (nx < 1 || ny < 1 || nx_f < 1 || ny_f < 1) { fprintf(stderr, "bad extents\n"); return 2; }
    const size_t n = (size_t)nx * ny, nf = (size_t)nx_f * ny_f;
    int *x = take(4 * n * sizeof(int)), *y = take(4 * n * sizeof(int));
    float *w = take(4 * n * sizeof(float)), *lo = take(nf * sizeof(float));
    if (f) {
        get(x, 4 * n * sizeof(int), f); get(y, 4 * n * sizeof(int), f); get(w, 4 * n * sizeof(float), f); get(lo, nf * sizeof(float), f);
        fclose(f);
    } else {
        for (size_t c = 0; c < n; ++c)
            for (int l = 0; l < 4; ++l) {
                x[4 * c + l] = 1 + (int)((c + (size_t)l) % (size_t)nx_f);          /* both columns and both rows, in every position */
                y[4 * c + l] = 1 + (int)((c / 2 + (size_t)(l / 2)) % (size_t)ny_f);
                w[4 * c + l] = l == 3 ? 1.0e30f : 0.25f + 0.125f * (float)l;       /* w(4) is never read */
            }
        for (size_t t = 0; t < nf; ++t) lo[t] = 280.0f + (float)t;
    }
    for (size_t t = 0; t < 4 * n; ++t)
        if (x[t] < 1 || x[t] > nx_f || y[t] < 1 || y[t] > ny_f) { fprintf(stderr, "a table index outside the forcing grid\n"); return 2; }
    float *data = take(n * sizeof(float)), *dqdt = take(n * sizeof(float));
    double *acc = take(n * sizeof(double));
    for (size_t c = 0; c < n; ++c) {
        data[c] = f2_geo_cell(lo, nx_f, x + 4 * c, y + 4 * c, w + 4 * c);
        dqdt[c] = data[c] + 1.5f;
        acc[c] = (double)c;
    }
    if (argc > 2) {
        FILE *o = fopen(argv[2], "wb");
        if (!o || fwrite(data, sizeof(float), n, o) != n) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        fclose(o);
    }
    double sum = 0.0;
    for (size_t c = 0; c < n; ++c) {
        dqdt[c] = f2_delta(dqdt[c], data[c], 3600.0);
        data[c] = f2_apply(data[c], dqdt[c], 17.3);
        acc[c] = f2_precip(acc[c], data[c], 17.3);
        sum += acc[c];
    }
    printf("forcing2d_bounds: %d x %d from %d x %d, sum %.17g\n", nx, ny, nx_f, ny_f, sum);
    free(x); free(y); free(w); free(lo); free(data); free(dqdt); free(acc);
    return 0;
}
