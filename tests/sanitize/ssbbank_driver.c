/* Host-only exercise of the SSBBank's C ABI (ldsp_ssbbank_*) under ASan / UBSan,
 * linked against the instrumented library of `make asan` and built by
 * `make -C python-liquiddsp_amd ssbbank_asan`; run without a GPU by
 * tests/test_ssbbank_host.py.  Covers create over the corners of the supported
 * (C, D, L) range with the default and explicit bands and lengths, the rows'
 * complex taps (|g_c[j]| = |p[j]|, L = 1025 rows of 256), every rejected
 * argument, create_taps at the shortest and longest prototypes, get_info /
 * get_band / get_taps / get_words / get_bfo / set_bfo / get_sideband /
 * set_sideband, num_outputs, the tile and the seek hook, every argument error of
 * execute (decided on the host), reset before any device work, and destroy.
 * Exit status 0 = every check held; the sanitizers abort on the first report. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ldsp.h"

static int fails = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) {                                                                 \
            fprintf(stderr, "check failed at %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, \
                    ldsp_last_error());                                             \
            fails++;                                                                \
        }                                                                           \
    } while (0)

static double bfo[257];
static int side[257];

static void lists(void)
{
    for (int c = 0; c < 257; c++) {
        bfo[c] = -0.5 + (double)c / 256.0;               /* -0.5 .. 0.5, both ends */
        side[c] = c % 2 ? -1 : 1;
    }
}

static void designs(void)
{
    const unsigned Ds[] = {1, 4, 5, 32}, Cs[] = {1, 3, 256}, Ls[] = {0, 1, 33, 1025};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 3; j++)
            for (int l = 0; l < 4; l++) {
                const unsigned D = Ds[i], C = Cs[j], want = Ls[l] ? Ls[l] : 1001;
                ldsp_ssbbank_t q = NULL;
                CHECK(ldsp_ssbbank_create(C, D, 0.002, 0.015, Ls[l], 60.0f, bfo, side, &q) == LDSP_OK && q != NULL);
                unsigned Co = 0, Do = 0, L = 0, skip = 99;
                CHECK(ldsp_ssbbank_get_info(q, &Co, &Do, &L, &skip) == LDSP_OK);
                CHECK(Co == C && Do == D && L == want && skip == 0);
                CHECK(ldsp_ssbbank_get_info(q, NULL, NULL, NULL, NULL) == LDSP_OK);
                double lo = 0.0, hi = 0.0;
                CHECK(ldsp_ssbbank_get_band(q, &lo, &hi) == LDSP_OK && lo == 0.002 && hi == 0.015);
                CHECK(ldsp_ssbbank_get_band(q, NULL, NULL) == LDSP_OK);
                float *p = (float *)malloc((size_t)L * sizeof(float));
                float *g = (float *)malloc(2 * (size_t)C * L * sizeof(float));
                CHECK(ldsp_ssbbank_get_taps(q, p, g) == LDSP_OK);
                CHECK(ldsp_ssbbank_get_taps(q, NULL, NULL) == LDSP_OK);
                double sp = 0.0;
                for (unsigned k = 0; k < L; k++) sp += (double)p[k];
                CHECK(fabs(sp - 1.0) < 1e-6);
                for (unsigned c = 0; c < C; c++)
                    for (unsigned k = 0; k < L; k++) {   /* a rotation of p[k], rounded once per component */
                        const double m = hypot((double)g[2 * (c * L + k)], (double)g[2 * (c * L + k) + 1]);
                        CHECK(fabs(m - fabs((double)p[k])) <= 1.5e-7 * fabs((double)p[k]));
                    }
                uint32_t *w = (uint32_t *)malloc(C * sizeof(uint32_t));
                double *b = (double *)malloc(C * sizeof(double));
                int *s = (int *)malloc(C * sizeof(int));
                CHECK(ldsp_ssbbank_get_words(q, w) == LDSP_OK && w[0] == 0x80000000u);
                CHECK(ldsp_ssbbank_get_bfo(q, b) == LDSP_OK && memcmp(b, bfo, C * sizeof(double)) == 0);
                CHECK(ldsp_ssbbank_get_sideband(q, s) == LDSP_OK && memcmp(s, side, C * sizeof(int)) == 0);
                CHECK(ldsp_ssbbank_set_bfo(q, bfo + 1) == LDSP_OK && ldsp_ssbbank_set_sideband(q, side + 1) == LDSP_OK);
                CHECK(ldsp_ssbbank_get_bfo(q, b) == LDSP_OK && memcmp(b, bfo + 1, C * sizeof(double)) == 0);
                CHECK(ldsp_ssbbank_get_sideband(q, s) == LDSP_OK && memcmp(s, side + 1, C * sizeof(int)) == 0);
                CHECK(ldsp_ssbbank_get_words(q, w) == LDSP_OK && w[0] == 0x81000000u);
                free(s);
                free(b);
                free(w);
                size_t n = 99;
                CHECK(ldsp_ssbbank_num_outputs(q, 0, &n) == LDSP_OK && n == 0);
                CHECK(ldsp_ssbbank_num_outputs(q, 3 * (size_t)D + 1, &n) == LDSP_OK && n == 4);
                size_t cols = 0;
                CHECK(ldsp_debug_ssbbank_tile(D, L, &cols) == LDSP_OK && cols == 128);
                free(g);
                free(p);
                const uint64_t T = ((uint64_t)3 << 32) + 5;
                CHECK(ldsp_debug_ssbbank_seek(q, T) == LDSP_OK);
                CHECK(ldsp_ssbbank_get_info(q, NULL, NULL, NULL, &skip) == LDSP_OK && skip == (D - T % D) % D);
                CHECK(ldsp_ssbbank_reset(q) == LDSP_OK);
                CHECK(ldsp_ssbbank_get_info(q, NULL, NULL, NULL, &skip) == LDSP_OK && skip == 0);
                CHECK(ldsp_ssbbank_destroy(q) == LDSP_OK);
            }
    ldsp_ssbbank_t q = NULL;
    CHECK(ldsp_ssbbank_create(2, 4, 1.0 / 512.0, 0.0, 0, 40.0f, bfo, side, &q) == LDSP_OK);
    unsigned L = 0;
    double lo = 0.0, hi = 0.0;
    CHECK(ldsp_ssbbank_get_info(q, NULL, NULL, &L, NULL) == LDSP_OK && L == 1025);
    CHECK(ldsp_ssbbank_get_band(q, &lo, &hi) == LDSP_OK && lo == 1.0 / 512.0 && hi == 0.125 - 1.0 / 512.0);
    CHECK(ldsp_ssbbank_destroy(q) == LDSP_OK);
    CHECK(ldsp_ssbbank_destroy(NULL) == LDSP_OK);
}

static void rejected(void)
{
    ldsp_ssbbank_t q = NULL;
    double bad[3] = {0.0, 0.6, 0.0}, nanb[3] = {0.0, 0.0, NAN};
    int zero[3] = {1, 0, 1}, two[3] = {1, -1, 2};
    CHECK(ldsp_ssbbank_create(0, 2, 0.025, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL && q == NULL);
    CHECK(ldsp_ssbbank_create(257, 2, 0.025, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 0, 0.025, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 33, 0.002, 0.01, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.0, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, -0.025, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.125, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);   /* the default hi = lo */
    CHECK(ldsp_ssbbank_create(3, 32, 0.025, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);  /* the default hi < lo */
    CHECK(ldsp_ssbbank_create(3, 2, 0.1, 0.1, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.2501, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, -0.1, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, NAN, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, NAN, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, INFINITY, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 1026, 60.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 0.0f, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, NAN, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0f, bad, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0f, nanb, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0f, bfo, zero, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0f, bfo, two, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0f, NULL, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0f, bfo, NULL, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0f, bfo, side, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create(3, 4, 0.0019, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_EUNSUP);  /* default L = 1055 */
    CHECK(q == NULL && strlen(ldsp_last_error()) > 0);
    CHECK(ldsp_ssbbank_create(3, 4, 0.0019, 0.0, 0, 60.0f, bad, side, &q) == LDSP_EINVAL);  /* out of range comes first */
    CHECK(ldsp_ssbbank_create(3, 4, 0.0019, 0.0, 1025, 60.0f, bfo, side, &q) == LDSP_OK);
    CHECK(ldsp_ssbbank_set_bfo(q, bad) == LDSP_EINVAL && ldsp_ssbbank_set_bfo(q, nanb) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_set_sideband(q, zero) == LDSP_EINVAL && ldsp_ssbbank_set_sideband(q, two) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_set_bfo(q, NULL) == LDSP_EINVAL && ldsp_ssbbank_set_sideband(q, NULL) == LDSP_EINVAL);
    double b[3];
    int s[3];
    CHECK(ldsp_ssbbank_get_bfo(q, b) == LDSP_OK && memcmp(b, bfo, sizeof b) == 0);          /* refused lists change nothing */
    CHECK(ldsp_ssbbank_get_sideband(q, s) == LDSP_OK && memcmp(s, side, sizeof s) == 0);
    CHECK(ldsp_ssbbank_destroy(q) == LDSP_OK);
    q = NULL;

    static float p[1026];
    for (int i = 0; i < 1026; i++) p[i] = 1.0f / (float)(i + 1);
    CHECK(ldsp_ssbbank_create_taps(3, 2, p, 0, 0.025, 0.0, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 2, p, 1026, 0.025, 0.0, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 2, NULL, 8, 0.025, 0.0, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 2, p, 8, 0.025, 0.0, NULL, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 2, p, 8, 0.025, 0.0, bfo, NULL, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 2, p, 8, 0.025, 0.0, bfo, side, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(0, 2, p, 8, 0.025, 0.0, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(257, 2, p, 8, 0.025, 0.0, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 0, p, 8, 0.025, 0.0, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 33, p, 8, 0.002, 0.01, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 2, p, 8, 0.0, 0.0, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 2, p, 8, 0.025, 0.3, bfo, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 2, p, 8, 0.025, 0.0, bad, side, &q) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_create_taps(3, 2, p, 8, 0.025, 0.0, bfo, two, &q) == LDSP_EINVAL);
    CHECK(q == NULL);
    size_t cols = 0;
    CHECK(ldsp_debug_ssbbank_tile(0, 8, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ssbbank_tile(33, 8, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ssbbank_tile(8, 0, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ssbbank_tile(8, 1026, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ssbbank_tile(8, 8, NULL) == LDSP_EINVAL);
    CHECK(ldsp_debug_ssbbank_seek(NULL, 5) == LDSP_EINVAL);
}

static void user_taps_and_execute_errors(int ndev)
{
    static float p[1025], a[1025], g[3 * 2 * 1025];
    for (int i = 0; i < 1025; i++) p[i] = 0.01f * (float)(i % 13) - 0.05f;
    const unsigned lens[] = {1, 5, 37, 1025};
    for (int i = 0; i < 4; i++) {
        ldsp_ssbbank_t q = NULL;
        CHECK(ldsp_ssbbank_create_taps(3, 8, p, lens[i], 0.01, 0.05, bfo + 100, side, &q) == LDSP_OK);
        unsigned L = 0;
        CHECK(ldsp_ssbbank_get_info(q, NULL, NULL, &L, NULL) == LDSP_OK && L == lens[i]);
        CHECK(ldsp_ssbbank_get_taps(q, a, g) == LDSP_OK);
        CHECK(memcmp(a, p, L * sizeof(float)) == 0);
        if (L == 1) CHECK(g[0] == p[0] && g[1] == 0.0f); /* psi = 0 */
        CHECK(ldsp_ssbbank_destroy(q) == LDSP_OK);
    }

    ldsp_ssbbank_t q = NULL;
    CHECK(ldsp_ssbbank_create(3, 4, 0.025, 0.0, 0, 60.0f, bfo, side, &q) == LDSP_OK);
    static float x[3 * 64 * 2], y[3 * 20];
    size_t k = 0;
    /* ldy < ncols: *ncols is set, with and without the pointer, and nothing is consumed */
    CHECK(ldsp_ssbbank_execute(q, x, 64, 64, y, 15, &k, LDSP_MEM_HOST, NULL) == LDSP_ERANGE && k == 16);
    CHECK(ldsp_ssbbank_execute(q, x, 64, 64, y, 0, NULL, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
    CHECK(ldsp_ssbbank_execute(q, x, 63, 64, y, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_execute(NULL, x, 64, 64, y, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_execute(q, NULL, 64, 64, y, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_execute(q, x, 64, 64, NULL, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_execute(q, x, 64, 64, y, 20, &k, 7, NULL) == LDSP_EINVAL && k == 16);
    CHECK(strstr(ldsp_last_error(), "mem") != NULL);
    if (ndev == 0) {                                     /* valid arguments: no device, no CPU fallback */
        CHECK(ldsp_ssbbank_execute(q, x, 64, 64, y, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EHIP);
        CHECK(strstr(ldsp_last_error(), "no CPU fallback") != NULL);
        CHECK(ldsp_ssbbank_execute(q, NULL, 0, 0, NULL, 0, &k, LDSP_MEM_HOST, NULL) == LDSP_EHIP && k == 0);
    }
    unsigned skip = 9;
    CHECK(ldsp_ssbbank_get_info(q, NULL, NULL, NULL, &skip) == LDSP_OK && skip == 0);
    CHECK(ldsp_ssbbank_num_outputs(q, 64, &k) == LDSP_OK && k == 16);
    CHECK(ldsp_ssbbank_num_outputs(q, 16, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_num_outputs(NULL, 16, &k) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_get_taps(NULL, p, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_get_words(q, NULL) == LDSP_EINVAL && ldsp_ssbbank_get_words(NULL, (uint32_t *)x) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_get_bfo(q, NULL) == LDSP_EINVAL && ldsp_ssbbank_get_bfo(NULL, bfo) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_get_sideband(q, NULL) == LDSP_EINVAL && ldsp_ssbbank_get_sideband(NULL, side) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_set_bfo(NULL, bfo) == LDSP_EINVAL && ldsp_ssbbank_set_sideband(NULL, side) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_get_info(NULL, NULL, NULL, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_get_band(NULL, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_reset(NULL) == LDSP_EINVAL);
    CHECK(ldsp_ssbbank_reset(q) == LDSP_OK);
    CHECK(ldsp_ssbbank_destroy(q) == LDSP_OK);
}

int main(void)
{
    int ndev = -1;
    if (ldsp_device_count(&ndev) != LDSP_OK) ndev = 0;
    lists();
    designs();
    rejected();
    user_taps_and_execute_errors(ndev);
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
