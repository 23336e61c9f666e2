/* cavity_cpu.c -- single-core restatement of one cavity-grid update for tools/cavity_bench.py:
 * the occupancy of G^3 grid points over all atoms, the count of the open points, and the darts, each tested against
 * every grid point with no early exit.  Compiled by the tool with gcc -O2; timed on the host the tool runs on. */
#include <math.h>
#include <stdlib.h>

/* pos: [P][3] grid points; atoms: [n][3]; darts: [nd][3]; occ: [P] out.  Returns hits; *n_open out. */
int cavity_cpu_update(int P, const double *pos, int n, const double *atoms, int nd, const double *darts, double radius,
                      int *occ, int *n_open) {
    int open = 0, hits = 0;
    for (int g = 0; g < P; g++) {
        int c = 0;
        for (int a = 0; a < n; a++) {
            double r = 0;
            for (int p = 0; p < 3; p++) r += (pos[3 * g + p] - atoms[3 * a + p]) * (pos[3 * g + p] - atoms[3 * a + p]);
            if (sqrt(r) < radius) ++c;
        }
        occ[g] = c;
        if (!c) ++open;
    }
    for (int d = 0; d < nd; d++) {
        int inside = 0;
        for (int g = 0; g < P; g++) {
            if (occ[g]) continue;
            double r = 0;
            for (int p = 0; p < 3; p++) r += (darts[3 * d + p] - pos[3 * g + p]) * (darts[3 * d + p] - pos[3 * g + p]);
            if (sqrt(r) < radius) inside = 1;
        }
        hits += inside;
    }
    *n_open = open;
    return hits;
}
