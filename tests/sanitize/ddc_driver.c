/* Host-only exercise of the Downconverter's C ABI (ldsp_ddc_*) under ASan /
 * UBSan, linked against the instrumented library of `make asan` and built by
 * `make -C python-liquiddsp_amd ddc_asan`; run without a GPU by
 * tests/test_downconverter_host.py.  Covers create over the corners of the
 * supported (C, D, m) range and every rejected argument, the frequency words,
 * create_taps at the shortest and longest prototypes, set_frequencies with a
 * changed tuner count, get_info / get_words / get_taps / get_scale / set_scale,
 * num_outputs, the tile hook, every argument error of execute (decided on the
 * host), seek and reset before any device work, and destroy.  Exit status 0 =
 * every check held; the sanitizers abort on the first report. */
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
    double f[64];
    for (int c = 0; c < 64; c++) f[c] = (double)c / 64.0 - 0.5;
    const unsigned Ds[] = {2, 5, 64, 100, 256}, Cs[] = {1, 2, 3, 64};
    for (int i = 0; i < 5; i++)
        for (int j = 0; j < 4; j++)
            for (unsigned m = 1; m <= 8; m += 7) {
                const unsigned D = Ds[i], C = Cs[j];
                ldsp_ddc_t q = NULL;
                CHECK(ldsp_ddc_create(f, C, D, m, 0.0f, 60.0f, &q) == LDSP_OK && q != NULL);
                unsigned Co = 0, Do = 0, L = 0, skip = 99;
                CHECK(ldsp_ddc_get_info(q, &Co, &Do, &L, &skip) == LDSP_OK);
                CHECK(Co == C && Do == D && L == 2 * D * m + 1 && skip == 0);
                CHECK(ldsp_ddc_get_info(q, NULL, NULL, NULL, NULL) == LDSP_OK);
                float *h = (float *)malloc(L * sizeof(float));
                CHECK(ldsp_ddc_get_taps(q, h) == LDSP_OK);
                double sum = 0.0;
                for (unsigned k = 0; k < L; k++) sum += (double)h[k];
                float s = 0.0f;
                CHECK(ldsp_ddc_get_scale(q, &s) == LDSP_OK && s == (float)(1.0 / sum));
                CHECK(h[L / 2] > 0.0f && isfinite(sum));
                free(h);
                CHECK(ldsp_ddc_set_scale(q, 0.5f) == LDSP_OK);
                CHECK(ldsp_ddc_get_scale(q, &s) == LDSP_OK && s == 0.5f);
                uint32_t w[64];
                CHECK(ldsp_ddc_get_words(q, w) == LDSP_OK);
                for (unsigned c = 0; c < C; c++) CHECK(w[c] == (uint32_t)((c << 26) ^ 0x80000000u));
                size_t n = 99;
                CHECK(ldsp_ddc_num_outputs(q, 0, &n) == LDSP_OK && n == 0);
                CHECK(ldsp_ddc_num_outputs(q, 3 * (size_t)D + 1, &n) == LDSP_OK && n == 4);
                size_t cols = 0;
                CHECK(ldsp_debug_ddc_tile(D, L, &cols) == LDSP_OK && (cols == 32 || cols == 64));
                /* the stream position alone moves the schedule; nothing is on the device yet */
                CHECK(ldsp_debug_ddc_seek(q, ((uint64_t)1 << 32) - 1) == LDSP_OK);
                CHECK(ldsp_ddc_get_info(q, NULL, NULL, NULL, &skip) == LDSP_OK);
                CHECK(skip == (D - (unsigned)((((uint64_t)1 << 32) - 1) % D)) % D);
                CHECK(ldsp_ddc_reset(q) == LDSP_OK);
                CHECK(ldsp_ddc_get_info(q, NULL, NULL, NULL, &skip) == LDSP_OK && skip == 0);
                CHECK(ldsp_ddc_destroy(q) == LDSP_OK);
            }
    ldsp_ddc_t q = NULL;
    CHECK(ldsp_ddc_create(f, 4, 16, 4, 0.05f, 40.0f, &q) == LDSP_OK);
    /* retune: fewer, then more tuners */
    const double g[5] = {0.0, 0.5, -0.5, 1.0, 0x1p-32};
    uint32_t w[5] = {9, 9, 9, 9, 9};
    unsigned C = 0;
    CHECK(ldsp_ddc_set_frequencies(q, g, 1) == LDSP_OK);
    CHECK(ldsp_ddc_get_info(q, &C, NULL, NULL, NULL) == LDSP_OK && C == 1);
    CHECK(ldsp_ddc_set_frequencies(q, g, 5) == LDSP_OK);
    CHECK(ldsp_ddc_get_info(q, &C, NULL, NULL, NULL) == LDSP_OK && C == 5);
    CHECK(ldsp_ddc_get_words(q, w) == LDSP_OK);
    CHECK(w[0] == 0 && w[1] == 0x80000000u && w[2] == 0x80000000u && w[3] == 0 && w[4] == 1);
    /* a rejected list leaves the old one */
    const double bad[2] = {0.25, 1.5};
    CHECK(ldsp_ddc_set_frequencies(q, bad, 2) == LDSP_EINVAL);
    CHECK(ldsp_ddc_set_frequencies(q, g, 0) == LDSP_EINVAL);
    CHECK(ldsp_ddc_set_frequencies(q, g, 65) == LDSP_EUNSUP);
    CHECK(ldsp_ddc_set_frequencies(q, NULL, 2) == LDSP_EINVAL);
    CHECK(ldsp_ddc_set_frequencies(NULL, g, 2) == LDSP_EINVAL);
    CHECK(ldsp_ddc_get_info(q, &C, NULL, NULL, NULL) == LDSP_OK && C == 5);
    CHECK(ldsp_ddc_destroy(q) == LDSP_OK);
    CHECK(ldsp_ddc_destroy(NULL) == LDSP_OK);
}

static void rejected(void)
{
    ldsp_ddc_t q = NULL;
    double f[65];
    for (int c = 0; c < 65; c++) f[c] = 0.001 * c;
    CHECK(ldsp_ddc_create(f, 2, 0, 6, 0.0f, 60.0f, &q) == LDSP_EINVAL && q == NULL);
    CHECK(ldsp_ddc_create(f, 2, 1, 6, 0.0f, 60.0f, &q) == LDSP_EUNSUP);
    CHECK(ldsp_ddc_create(f, 2, 257, 6, 0.0f, 60.0f, &q) == LDSP_EUNSUP);
    CHECK(ldsp_ddc_create(f, 0, 8, 6, 0.0f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create(f, 65, 8, 6, 0.0f, 60.0f, &q) == LDSP_EUNSUP);
    CHECK(ldsp_ddc_create(f, 2, 8, 0, 0.0f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create(f, 2, 8, 9, 0.0f, 60.0f, &q) == LDSP_EUNSUP);
    CHECK(ldsp_ddc_create(f, 2, 8, 6, 0.0f, 0.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create(f, 2, 8, 6, 0.5f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create(NULL, 2, 8, 6, 0.0f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create(f, 2, 8, 6, 0.0f, 60.0f, NULL) == LDSP_EINVAL);
    const double nf[4] = {NAN, INFINITY, 1.0000001, -1.5};
    for (int i = 0; i < 4; i++) CHECK(ldsp_ddc_create(&nf[i], 1, 8, 6, 0.0f, 60.0f, &q) == LDSP_EINVAL);
    CHECK(q == NULL && strlen(ldsp_last_error()) > 0);

    float h[17 * 8 + 1];
    for (int i = 0; i < 17 * 8 + 1; i++) h[i] = 1.0f / (float)(i + 1);
    CHECK(ldsp_ddc_create_taps(f, 2, 8, h, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create_taps(f, 2, 8, NULL, 8, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create_taps(f, 2, 8, h, 8, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create_taps(NULL, 2, 8, h, 8, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create_taps(f, 2, 0, h, 8, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create_taps(f, 2, 1, h, 8, &q) == LDSP_EUNSUP);
    CHECK(ldsp_ddc_create_taps(f, 2, 257, h, 8, &q) == LDSP_EUNSUP);
    CHECK(ldsp_ddc_create_taps(f, 0, 8, h, 8, &q) == LDSP_EINVAL);
    CHECK(ldsp_ddc_create_taps(f, 65, 8, h, 8, &q) == LDSP_EUNSUP);
    CHECK(ldsp_ddc_create_taps(f, 2, 8, h, 17 * 8 + 1, &q) == LDSP_EUNSUP);
    CHECK(q == NULL);
    size_t cols = 0;
    CHECK(ldsp_debug_ddc_tile(0, 8, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ddc_tile(1, 8, &cols) == LDSP_EUNSUP);
    CHECK(ldsp_debug_ddc_tile(257, 8, &cols) == LDSP_EUNSUP);
    CHECK(ldsp_debug_ddc_tile(8, 0, &cols) == LDSP_EINVAL);
    CHECK(ldsp_debug_ddc_tile(8, 17 * 8 + 1, &cols) == LDSP_EUNSUP);
    CHECK(ldsp_debug_ddc_tile(8, 8, NULL) == LDSP_EINVAL);
}

static void user_taps_and_execute_errors(int ndev)
{
    const double f[3] = {0.0371, -0.31337, 0.25};
    float h[17 * 8];
    for (int i = 0; i < 17 * 8; i++) h[i] = 0.01f * (float)(i % 13) - 0.05f;
    const unsigned lens[] = {1, 5, 37, 17 * 8};
    for (int i = 0; i < 4; i++) {
        ldsp_ddc_t q = NULL;
        CHECK(ldsp_ddc_create_taps(f, 3, 8, h, lens[i], &q) == LDSP_OK);
        unsigned L = 0;
        CHECK(ldsp_ddc_get_info(q, NULL, NULL, &L, NULL) == LDSP_OK && L == lens[i]);
        float out[17 * 8];
        CHECK(ldsp_ddc_get_taps(q, out) == LDSP_OK && memcmp(out, h, L * sizeof(float)) == 0);
        float s = 0.0f;
        CHECK(ldsp_ddc_get_scale(q, &s) == LDSP_OK && s == 1.0f);
        CHECK(ldsp_ddc_destroy(q) == LDSP_OK);
    }

    ldsp_ddc_t q = NULL;
    CHECK(ldsp_ddc_create(f, 3, 4, 6, 0.0f, 60.0f, &q) == LDSP_OK);
    static float x[64 * 2], y[3 * 20 * 2];
    size_t k = 0;
    /* ld < ncols: *ncols is set, with and without the pointer, and nothing is consumed */
    CHECK(ldsp_ddc_execute(q, x, 64, y, 15, &k, LDSP_MEM_HOST, NULL) == LDSP_ERANGE && k == 16);
    CHECK(ldsp_ddc_execute(q, x, 64, y, 0, NULL, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
    CHECK(ldsp_ddc_execute(NULL, x, 64, y, 16, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ddc_execute(q, NULL, 64, y, 16, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ddc_execute(q, x, 64, NULL, 16, &k, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ddc_execute(q, x, 64, y, 16, &k, 7, NULL) == LDSP_EINVAL);
    CHECK(strstr(ldsp_last_error(), "mem") != NULL);
    CHECK(ldsp_ddc_execute(q, x, 64, y, 20, &k, 7, NULL) == LDSP_EINVAL && k == 16);
    if (ndev == 0) {                                     /* valid arguments: no device, no CPU fallback */
        CHECK(ldsp_ddc_execute(q, x, 64, y, 16, &k, LDSP_MEM_HOST, NULL) == LDSP_EHIP);
        CHECK(strstr(ldsp_last_error(), "no CPU fallback") != NULL);
        CHECK(ldsp_ddc_execute(q, NULL, 0, NULL, 0, &k, LDSP_MEM_HOST, NULL) == LDSP_EHIP && k == 0);
    }
    unsigned skip = 9;
    CHECK(ldsp_ddc_get_info(q, NULL, NULL, NULL, &skip) == LDSP_OK && skip == 0);
    CHECK(ldsp_ddc_num_outputs(q, 64, &k) == LDSP_OK && k == 16);
    CHECK(ldsp_ddc_num_outputs(q, 16, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ddc_num_outputs(NULL, 16, &k) == LDSP_EINVAL);
    CHECK(ldsp_ddc_get_taps(q, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ddc_get_taps(NULL, h) == LDSP_EINVAL);
    CHECK(ldsp_ddc_get_words(q, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ddc_get_words(NULL, (uint32_t *)x) == LDSP_EINVAL);
    CHECK(ldsp_ddc_get_scale(q, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ddc_set_scale(NULL, 1.0f) == LDSP_EINVAL);
    CHECK(ldsp_ddc_get_info(NULL, NULL, NULL, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_ddc_reset(NULL) == LDSP_EINVAL);
    CHECK(ldsp_debug_ddc_seek(NULL, 5) == LDSP_EINVAL);
    CHECK(ldsp_debug_ddc_seek(q, ((uint64_t)1 << 40) + 7) == LDSP_OK);
    CHECK(ldsp_ddc_get_info(q, NULL, NULL, NULL, &skip) == LDSP_OK && skip == 1);
    CHECK(ldsp_ddc_num_outputs(q, 1, &k) == LDSP_OK && k == 0);
    CHECK(ldsp_ddc_num_outputs(q, 2, &k) == LDSP_OK && k == 1);
    CHECK(ldsp_ddc_reset(q) == LDSP_OK);
    CHECK(ldsp_ddc_destroy(q) == LDSP_OK);
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
