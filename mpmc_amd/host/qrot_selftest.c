/* qrot_selftest.c -- a stand-alone program over qrot.c alone (no device, no engine library): the hindered-rotor case of
 * `quantum_rotation` from the keyword checks to the printed levels, the placements of a two-site rotor, and the solver on
 * a matrix with degenerate pairs.  What `make qrot_selftest_asan` builds with -fsanitize=address,undefined and runs on the
 * CPU; exit status 0 = every check held.  The few symbols qrot.c takes from the rest of the host layer are defined here. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "mpmc_host.h"

void output(const char *msg) { fputs(msg, stdout); }
void error(const char *msg) { fputs(msg, stderr); }
static unsigned long long g_state = 88172645463325252ull;
double get_rand(system_t *system) { /* xorshift64: any generator on [0, 1) serves here */
    (void)system;
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
int energy_hip_trial_energies(system_t *system, molecule_t *molecule, int ntrial, const double *xyz, double *energy) {
    (void)system, (void)molecule, (void)ntrial, (void)xyz, (void)energy;
    return -1; /* the hindered rotor asks for no energy */
}

static int fail(const char *what) {
    fprintf(stderr, "qrot_selftest: %s\n", what);
    return 1;
}

int main(void) {
    system_t system;
    memset(&system, 0, sizeof(system));
    system.ensemble = ENSEMBLE_NVT;
    system.temperature = 50.0;
    system.quantum_rotation = system.quantum_rotation_hindered = 1;
    system.quantum_rotation_B = 85.35060622;
    system.quantum_rotation_hindered_barrier = 10.0;
    system.quantum_rotation_sum = 10;
    atom_t a[4];
    molecule_t m[2];
    memset(a, 0, sizeof(a));
    memset(m, 0, sizeof(m));
    for (int k = 0; k < 2; k++) {
        m[k].id = k + 1;
        strcpy(m[k].moleculetype, "H2");
        m[k].atoms = &a[2 * k];
        a[2 * k].next = &a[2 * k + 1];
        a[2 * k].mass = a[2 * k + 1].mass = 1.008;
        a[2 * k].pos[0] = 3.0 * k + 0.1;
        a[2 * k].pos[1] = -0.2;
        a[2 * k].pos[2] = 0.371;
        a[2 * k + 1].pos[0] = 3.0 * k - 0.1;
        a[2 * k + 1].pos[1] = 0.2;
        a[2 * k + 1].pos[2] = -0.371;
        for (int q = 0; q < 3; q++) m[k].com[q] = 0.5 * (a[2 * k].pos[q] + a[2 * k + 1].pos[q]);
    }
    m[0].next = &m[1];
    m[1].nuclear_spin = NUCLEAR_SPIN_ORTHO;
    system.molecules = m;
    for (int l_max = 1; l_max <= QROT_L_LIMIT; l_max++) { /* every basis size, the last level included */
        system.quantum_rotation_l_max = l_max;
        system.quantum_rotation_level_max = (l_max + 1) * (l_max + 1);
        if (system.quantum_rotation_sum > system.quantum_rotation_level_max) system.quantum_rotation_sum = system.quantum_rotation_level_max;
        if (qrot_check(&system)) return fail("the keyword block was refused");
        if (quantum_system_rotational_energies(&system)) return fail("the evaluation failed");
        for (int k = 0; k < 2; k++) {
            for (int i = 1; i < system.quantum_rotation_level_max; i++)
                if (!(m[k].quantum_rotational_energies[i] >= m[k].quantum_rotational_energies[i - 1])) return fail("levels not ascending");
            if (!(m[k].rot_partfunc > 0.0 && m[k].rot_partfunc < 1.0)) return fail("partition function ratio outside (0, 1)");
        }
        if (fabs(m[0].rot_partfunc + m[1].rot_partfunc - 1.0) > 1e-12) return fail("para + ortho ratios do not add up to 1");
        system.quantum_rotation_sum = 10;
    }
    system.quantum_rotation_l_max = 9;
    if (!qrot_check(&system)) return fail("l_max 9 was accepted");
    /* placements: 256 rigid copies about the centre of mass */
    double *xyz = malloc(256 * 2 * 3 * sizeof(double));
    if (!xyz || qrot_placements(&m[1], xyz) != 2) return fail("placements");
    for (int t = 0; t < 256; t++) {
        double d = 0, c = 0;
        for (int q = 0; q < 3; q++) {
            d += (xyz[6 * t + q] - xyz[6 * t + 3 + q]) * (xyz[6 * t + q] - xyz[6 * t + 3 + q]);
            c += fabs(0.5 * (xyz[6 * t + q] + xyz[6 * t + 3 + q]) - m[1].com[q]);
        }
        if (fabs(sqrt(d) - sqrt(0.04 + 0.16 + 0.742 * 0.742)) > 1e-12 || c > 1e-12) return fail("a placement is not rigid about the centre");
    }
    free(xyz);
    /* the solver on a 6 x 6 Hermitian matrix with two degenerate pairs: U diag(1, 1, 2, 3, 3, 7) U^H, U a product of plane
     * rotations with complex phases */
    enum { N = 6 };
    const double lam[N] = {1, 1, 2, 3, 3, 7};
    double u[N][N][2], h[N][N][2], eval[N], evec[N][N][2];
    memset(u, 0, sizeof(u));
    for (int i = 0; i < N; i++) u[i][i][0] = 1.0;
    for (int p = 0; p < N; p++)
        for (int q = p + 1; q < N; q++) {
            const double th = 0.3 + 0.37 * p + 0.11 * q, ph = 0.9 * p - 0.4 * q;
            for (int k = 0; k < N; k++) {
                const double pr = u[k][p][0], pi = u[k][p][1], qr = u[k][q][0], qi = u[k][q][1];
                const double er = cos(ph), ei = sin(ph);
                u[k][p][0] = cos(th) * pr - sin(th) * (qr * er + qi * ei);
                u[k][p][1] = cos(th) * pi - sin(th) * (qi * er - qr * ei);
                u[k][q][0] = sin(th) * (pr * er - pi * ei) + cos(th) * qr;
                u[k][q][1] = sin(th) * (pi * er + pr * ei) + cos(th) * qi;
            }
        }
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            h[i][j][0] = h[i][j][1] = 0;
            for (int k = 0; k < N; k++) {
                h[i][j][0] += lam[k] * (u[i][k][0] * u[j][k][0] + u[i][k][1] * u[j][k][1]);
                h[i][j][1] += lam[k] * (u[i][k][1] * u[j][k][0] - u[i][k][0] * u[j][k][1]);
            }
        }
    for (int i = 0; i < N; i++)
        for (int j = i; j < N; j++) { /* exactly Hermitian */
            h[j][i][0] = h[i][j][0];
            h[j][i][1] = -h[i][j][1];
            if (i == j) h[i][j][1] = 0;
        }
    long rotations = 0;
    if (qrot_jacobi(N, &h[0][0][0], eval, &evec[0][0][0], &rotations) < 0) return fail("the solver did not converge");
    for (int i = 0; i < N; i++)
        if (fabs(eval[i] - lam[i]) > 1e-12) return fail("eigenvalues of the degenerate matrix");
    printf("qrot_selftest: ok (%ld rotations on the 6 x 6 matrix)\n", rotations);
    return 0;
}
