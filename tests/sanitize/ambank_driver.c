/* Host-only exercise of the AMBank's C ABI (ldsp_ambank_*) under ASan / UBSan,
 * linked against the instrumented library of `make asan` and built by
 * `make -C python-liquiddsp_amd ambank_asan`; run without a GPU by
 * tests/test_ambank_host.py.  Covers create over the corners of the supported
 * (C, D, L) range with the default and explicit cut-offs and lengths, d = h - g,
 * every rejected argument, create_taps at the shortest and longest prototypes,
 * get_info / get_taps / get_threshold / set_threshold / get_carrier_level,
 * num_outputs, the tile hook, every argument error of execute (decided on the
 * host), reset before any device work, and destroy.  Exit status 0 = every
 * check held; the sanitizers abort on the first report. */
#include <math.h>
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

static void designs(void)
{
    const unsigned Ds[] = {1, 4, 5, 32}, Cs[] = {1, 3, 256}, Ls[] = {0, 1, 33, 1025};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 3; j++)
            for (int l = 0; l < 4; l++) {
                const unsigned D = Ds[i], C = Cs[j], want = Ls[l] ? Ls[l] : 1001;
                ldsp_ambank_t q = NULL;
                CHECK(ldsp_ambank_create(C, D, 0.0, 0.004, Ls[l], 60.0f, 0.0f, &q) == LDSP_OK && q != NULL);
                unsigned Co = 0, Do = 0, L = 0, skip = 99;
                CHECK(ldsp_ambank_get_info(q, &Co, &Do, &L, &skip) == LDSP_OK);
                CHECK(Co == C && Do == D && L == want && skip == 0);
                CHECK(ldsp_ambank_get_info(q, NULL, NULL, NULL, NULL) == LDSP_OK);
                float *h = (float *)malloc(3 * (size_t)L * sizeof(float)), *g = h + L, *d = g + L;
                CHECK(ldsp_ambank_get_taps(q, h, g, d) == LDSP_OK);
                CHECK(ldsp_ambank_get_taps(q, NULL, NULL, NULL) == LDSP_OK);
                double sh = 0.0, sg = 0.0;
                for (unsigned k = 0; k < L; k++) {
                    sh += (double)h[k];
                    sg += (double)g[k];
                    CHECK(d[k] == (float)((double)h[k] - (double)g[k]));
                }
                CHECK(fabs(sh - 1.0) < 1e-6 && fabs(sg - 1.0) < 1e-6);
                size_t n = 99;
                CHECK(ldsp_ambank_num_outputs(q, 0, &n) == LDSP_OK && n == 0);
                CHECK(ldsp_ambank_num_outputs(q, 3 * (size_t)D + 1, &n) == LDSP_OK && n == 4);
                size_t cols = 0;
                CHECK(ldsp_debug_ambank_tile(D, L, &cols) == LDSP_OK && cols == 64);
                float *lv = (float *)malloc(C * sizeof(float));
                for (unsigned c = 0; c < C; c++) lv[c] = -1.0f;
                CHECK(ldsp_ambank_get_carrier_level(q, lv) == LDSP_OK);
                for (unsigned c = 0; c < C; c++) CHECK(lv[c] == 0.0f);
                free(lv);
                free(h);
                CHECK(ldsp_ambank_reset(q) == LDSP_OK);
                CHECK(ldsp_ambank_destroy(q) == LDSP_OK);
            }
    ldsp_ambank_t q = NULL;
    CHECK(ldsp_ambank_create(2, 4, 0.125, 2.0 / 512.0, 0, 40.0f, 0.25f, &q) == LDSP_OK);
    unsigned L = 0;
    float t = -1.0f;
    CHECK(ldsp_ambank_get_info(q, NULL, NULL, &L, NULL) == LDSP_OK && L == 1025);
    CHECK(ldsp_ambank_get_threshold(q, &t) == LDSP_OK && t == 0.25f);
    CHECK(ldsp_ambank_set_threshold(q, 0.0f) == LDSP_OK);
    CHECK(ldsp_ambank_set_threshold(q, -0.5f) == LDSP_EINVAL);
    CHECK(ldsp_ambank_set_threshold(q, NAN) == LDSP_EINVAL);
    CHECK(ldsp_ambank_get_threshold(q, &t) == LDSP_OK && t == 0.0f);
    CHECK(ldsp_ambank_destroy(q) == LDSP_OK);
    CHECK(ldsp_ambank_destroy(NULL) == LDSP_OK);
}

static void rejected(void)
{
    ldsp_ambank_t q = NULL;
    CHECK(ldsp_ambank_create(0, 4, 0.0, 0.004, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL && q == NULL);
    CHECK(ldsp_ambank_create(257, 4, 0.0, 0.004, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 0, 0.0, 0.004, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 33, 0.0, 0.004, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.0, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, -0.004, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.125, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);      /* carrier = the default audio */
    CHECK(ldsp_ambank_create(2, 4, 0.1, 0.1, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.51, 0.004, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, -0.1, 0.004, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, NAN, 0.004, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, NAN, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, INFINITY, 0, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.004, 1026, 60.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.004, 0, 0.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.004, 0, NAN, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.004, 0, 60.0f, -0.1f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.004, 0, 60.0f, NAN, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.004, 0, 60.0f, 0.0f, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.003, 0, 60.0f, 0.0f, &q) == LDSP_EUNSUP);     /* default L = 1335 */
    CHECK(q == NULL && strlen(ldsp_last_error()) > 0);
    CHECK(ldsp_ambank_create(2, 4, 0.0, 0.003, 1025, 60.0f, 0.0f, &q) == LDSP_OK);
    CHECK(ldsp_ambank_destroy(q) == LDSP_OK);
    q = NULL;

    static float h[1026];
    for (int i = 0; i < 1026; i++) h[i] = 1.0f / (float)(i + 1);
    CHECK(ldsp_ambank_create_taps(2, 4, h, 0, h, 0, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(2, 4, h, 1026, h, 1026, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(2, 4, h, 8, h, 7, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(2, 4, NULL, 8, h, 8, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(2, 4, h, 8, NULL, 8, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(2, 4, h, 8, h, 8, 0.0f, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(0, 4, h, 8, h, 8, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(257, 4, h, 8, h, 8, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(2, 0, h, 8, h, 8, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(2, 33, h, 8, h, 8, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ambank_create_taps(2, 4, h, 8, h, 8, -1.0f, &q) == LDSP_EINVAL);
    CHECK(q == NULL);
    size_t cols = 0;
    CHECK(ldsp_debug_ambank_tile(0, 8, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ambank_tile(33, 8, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ambank_tile(8, 0, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ambank_tile(8, 1026, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ambank_tile(8, 8, NULL) == LDSP_EINVAL);
}

static void user_taps_and_execute_errors(int ndev)
{
    static float h[1025], g[1025], a[1025], b[1025], d[1025];
    for (int i = 0; i < 1025; i++) {
        h[i] = 0.01f * (float)(i % 13) - 0.05f;
        g[i] = 0.003f * (float)(i % 7);
    }
    const unsigned lens[] = {1, 5, 37, 1025};
    for (int i = 0; i < 4; i++) {
        ldsp_ambank_t q = NULL;
        CHECK(ldsp_ambank_create_taps(3, 8, h, lens[i], g, lens[i], 0.01f, &q) == LDSP_OK);
        unsigned L = 0;
        CHECK(ldsp_ambank_get_info(q, NULL, NULL, &L, NULL) == LDSP_OK && L == lens[i]);
        CHECK(ldsp_ambank_get_taps(q, a, b, d) == LDSP_OK);
        CHECK(memcmp(a, h, L * sizeof(float)) == 0 && memcmp(b, g, L * sizeof(float)) == 0);
        for (unsigned k = 0; k < L; k++) CHECK(d[k] == (float)((double)h[k] - (double)g[k]));
        CHECK(ldsp_ambank_destroy(q) == LDSP_OK);
    }

    ldsp_ambank_t q = NULL;
    CHECK(ldsp_ambank_create(3, 4, 0.0, 0.016, 0, 60.0f, 0.0f, &q) == LDSP_OK);
    static float x[3 * 64 * 2], y[3 * 20];
    size_t k = 0;
    /* ldy < ncols: *ncols is set, with and without the pointer, and nothing is consumed */
    CHECK(ldsp_ambank_execute(q, x, 64, 64, y, 15, &k, LDSP_MEM_HOST, NULL) == LDSP_ERANGE && k == 16);
    CHECK(ldsp_ambank_execute(q, x, 64, 64, y, 0, NULL, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
    CHECK(ldsp_ambank_execute(q, x, 63, 64, y, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_execute(NULL, x, 64, 64, y, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_execute(q, NULL, 64, 64, y, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_execute(q, x, 64, 64, NULL, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_execute(q, x, 64, 64, y, 20, &k, 7, NULL) == LDSP_EINVAL && k == 16);
    CHECK(strstr(ldsp_last_error(), "mem") != NULL);
    if (ndev == 0) {                                     /* valid arguments: no device, no CPU fallback */
        CHECK(ldsp_ambank_execute(q, x, 64, 64, y, 20, &k, LDSP_MEM_HOST, NULL) == LDSP_EHIP);
        CHECK(strstr(ldsp_last_error(), "no CPU fallback") != NULL);
        CHECK(ldsp_ambank_execute(q, NULL, 0, 0, NULL, 0, &k, LDSP_MEM_HOST, NULL) == LDSP_EHIP && k == 0);
    }
    unsigned skip = 9;
    CHECK(ldsp_ambank_get_info(q, NULL, NULL, NULL, &skip) == LDSP_OK && skip == 0);
    CHECK(ldsp_ambank_num_outputs(q, 64, &k) == LDSP_OK && k == 16);
    CHECK(ldsp_ambank_num_outputs(q, 16, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_num_outputs(NULL, 16, &k) == LDSP_EINVAL);
    CHECK(ldsp_ambank_get_taps(NULL, h, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_get_threshold(q, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_get_threshold(NULL, h) == LDSP_EINVAL);
    CHECK(ldsp_ambank_set_threshold(NULL, 1.0f) == LDSP_EINVAL);
    CHECK(ldsp_ambank_get_carrier_level(q, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_get_carrier_level(NULL, h) == LDSP_EINVAL);
    CHECK(ldsp_ambank_get_info(NULL, NULL, NULL, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_reset(NULL) == LDSP_EINVAL);
    CHECK(ldsp_ambank_reset(q) == LDSP_OK);
    CHECK(ldsp_ambank_destroy(q) == LDSP_OK);
}

int main(void)
{
    int ndev = -1;
    if (ldsp_device_count(&ndev) != LDSP_OK) ndev = 0;
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
