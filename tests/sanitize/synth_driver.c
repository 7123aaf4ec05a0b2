/* Host-only exercise of the Synthesizer's C ABI (ldsp_synth_*) under ASan /
 * UBSan, linked against the instrumented library of `make asan` and built by
 * `make -C python-liquiddsp_amd synth_asan`; run without a GPU by
 * tests/test_synthesizer_host.py.  Covers create over every supported shape and
 * every rejected one, create_taps at the shortest and longest prototypes,
 * get_info / get_taps / get_scale / set_scale, num_outputs, reset before any
 * device work, every argument error of execute (decided on the host) and
 * destroy.  Exit status 0 = every check held; the sanitizers abort on the first
 * report. */
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
    for (unsigned M = 4; M <= 256; M *= 2)
        for (unsigned D = M / 2; D <= M; D += M / 2)
            for (unsigned m = 1; m <= 8; m += 7) {
                ldsp_synth_t q = NULL;
                CHECK(ldsp_synth_create(M, D, m, 0.0f, 60.0f, &q) == LDSP_OK && q != NULL);
                unsigned Mo = 0, Do = 0, L = 0;
                CHECK(ldsp_synth_get_info(q, &Mo, &Do, &L) == LDSP_OK);
                CHECK(Mo == M && Do == D && L == 2 * M * m + 1);
                CHECK(ldsp_synth_get_info(q, NULL, NULL, NULL) == LDSP_OK);
                float *g = (float *)malloc(L * sizeof(float));
                CHECK(ldsp_synth_get_taps(q, g) == LDSP_OK);
                double sum = 0.0;
                for (unsigned i = 0; i < L; i++) sum += (double)g[i];
                float s = 0.0f;
                CHECK(ldsp_synth_get_scale(q, &s) == LDSP_OK && s == (float)((double)D / sum));
                CHECK(g[L / 2] > 0.0f && isfinite(sum));
                free(g);
                CHECK(ldsp_synth_set_scale(q, 0.5f) == LDSP_OK);
                CHECK(ldsp_synth_get_scale(q, &s) == LDSP_OK && s == 0.5f);
                size_t n = 99;
                CHECK(ldsp_synth_num_outputs(q, 0, &n) == LDSP_OK && n == 0);
                CHECK(ldsp_synth_num_outputs(q, 37, &n) == LDSP_OK && n == 37 * (size_t)D);
                CHECK(ldsp_synth_reset(q) == LDSP_OK);       /* nothing on the device yet */
                size_t cols = 0;
                CHECK(ldsp_debug_synth_tile(M, D, &cols) == LDSP_OK && cols >= 32);
                CHECK(ldsp_synth_destroy(q) == LDSP_OK);
            }
    ldsp_synth_t q = NULL;
    CHECK(ldsp_synth_create(16, 8, 4, 0.05f, 40.0f, &q) == LDSP_OK);
    CHECK(ldsp_synth_destroy(q) == LDSP_OK);
    CHECK(ldsp_synth_destroy(NULL) == LDSP_OK);
}

static void rejected(void)
{
    ldsp_synth_t q = NULL;
    const unsigned bad[] = {0, 2, 3, 12};
    for (int i = 0; i < 4; i++) {
        CHECK(ldsp_synth_create(bad[i], bad[i], 6, 0.0f, 60.0f, &q) == LDSP_EINVAL && q == NULL);
        CHECK(ldsp_synth_create(bad[i], bad[i] / 2, 6, 0.0f, 60.0f, &q) == LDSP_EINVAL && q == NULL);
    }
    CHECK(ldsp_synth_create(16, 0, 6, 0.0f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create(16, 4, 6, 0.0f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create(16, 32, 6, 0.0f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create(16, 8, 0, 0.0f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create(16, 8, 6, 0.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create(16, 8, 6, 0.5f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create(16, 8, 6, 0.0f, 60.0f, NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_create(512, 256, 6, 0.0f, 60.0f, &q) == LDSP_EUNSUP);
    CHECK(ldsp_synth_create(16, 8, 9, 0.0f, 60.0f, &q) == LDSP_EUNSUP);
    CHECK(q == NULL && strlen(ldsp_last_error()) > 0);

    float g[17 * 8 + 1];
    for (int i = 0; i < 17 * 8 + 1; i++) g[i] = 1.0f / (float)(i + 1);
    CHECK(ldsp_synth_create_taps(8, 4, g, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create_taps(8, 4, NULL, 8, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create_taps(8, 4, g, 8, NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_create_taps(12, 6, g, 8, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create_taps(8, 2, g, 8, &q) == LDSP_EINVAL);
    CHECK(ldsp_synth_create_taps(512, 512, g, 8, &q) == LDSP_EUNSUP);
    CHECK(ldsp_synth_create_taps(8, 4, g, 17 * 8 + 1, &q) == LDSP_EUNSUP);
    CHECK(q == NULL);
    size_t cols = 0;
    CHECK(ldsp_debug_synth_tile(12, 6, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_synth_tile(16, 4, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_synth_tile(512, 256, &cols) == LDSP_EUNSUP);
    CHECK(ldsp_debug_synth_tile(16, 8, NULL) == LDSP_EINVAL);
}

static void user_taps_and_execute_errors(int ndev)
{
    float g[17 * 8];
    for (int i = 0; i < 17 * 8; i++) g[i] = 0.01f * (float)(i % 13) - 0.05f;
    const unsigned lens[] = {1, 5, 37, 17 * 8};
    for (int i = 0; i < 4; i++) {
        ldsp_synth_t q = NULL;
        CHECK(ldsp_synth_create_taps(8, i & 1 ? 4 : 8, g, lens[i], &q) == LDSP_OK);
        unsigned L = 0;
        CHECK(ldsp_synth_get_info(q, NULL, NULL, &L) == LDSP_OK && L == lens[i]);
        float out[17 * 8];
        CHECK(ldsp_synth_get_taps(q, out) == LDSP_OK && memcmp(out, g, L * sizeof(float)) == 0);
        float s = 0.0f;
        CHECK(ldsp_synth_get_scale(q, &s) == LDSP_OK && s == 1.0f);
        CHECK(ldsp_synth_destroy(q) == LDSP_OK);
    }

    ldsp_synth_t q = NULL;
    CHECK(ldsp_synth_create(8, 4, 6, 0.0f, 60.0f, &q) == LDSP_OK);
    static float y[8 * 16 * 2], z[16 * 4 * 2];
    size_t n = 0;
    /* ld < ncols */
    CHECK(ldsp_synth_execute(q, y, 15, 16, z, 64, &n, LDSP_MEM_HOST, NULL) == LDSP_EINVAL && n == 64);
    /* too small a capacity: *n is set, with and without the pointer */
    n = 0;
    CHECK(ldsp_synth_execute(q, y, 16, 16, z, 63, &n, LDSP_MEM_HOST, NULL) == LDSP_ERANGE && n == 64);
    CHECK(ldsp_synth_execute(q, y, 16, 16, z, 0, NULL, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
    CHECK(ldsp_synth_execute(NULL, y, 16, 16, z, 64, &n, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_execute(q, NULL, 16, 16, z, 64, &n, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_execute(q, y, 16, 16, NULL, 64, &n, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_execute(q, y, 16, 16, z, 64, &n, 7, NULL) == LDSP_EINVAL);
    CHECK(strstr(ldsp_last_error(), "mem") != NULL);
    /* the same with rows ld > ncols apart: still decided before the image is touched */
    CHECK(ldsp_synth_execute(q, y, 20, 16, z, 64, &n, 7, NULL) == LDSP_EINVAL && n == 64);
    if (ndev == 0) {                                     /* valid arguments: no device, no CPU fallback */
        CHECK(ldsp_synth_execute(q, y, 16, 16, z, 64, &n, LDSP_MEM_HOST, NULL) == LDSP_EHIP);
        CHECK(strstr(ldsp_last_error(), "no CPU fallback") != NULL);
        CHECK(ldsp_synth_execute(q, NULL, 0, 0, NULL, 0, &n, LDSP_MEM_HOST, NULL) == LDSP_EHIP && n == 0);
    }
    CHECK(ldsp_synth_num_outputs(q, 16, NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_num_outputs(NULL, 16, &n) == LDSP_EINVAL);
    CHECK(ldsp_synth_get_taps(q, NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_get_taps(NULL, g) == LDSP_EINVAL);
    CHECK(ldsp_synth_get_scale(q, NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_set_scale(NULL, 1.0f) == LDSP_EINVAL);
    CHECK(ldsp_synth_get_info(NULL, NULL, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_reset(NULL) == LDSP_EINVAL);
    CHECK(ldsp_synth_reset(q) == LDSP_OK);
    CHECK(ldsp_synth_destroy(q) == LDSP_OK);
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
