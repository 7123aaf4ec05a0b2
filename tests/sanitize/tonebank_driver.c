/* Host-only exercise of the ToneBank's C ABI (ldsp_tonebank_*) under ASan / UBSan,
 * linked against the instrumented library of `make asan` and built by
 * `make -C python-liquiddsp_amd tonebank_asan`; run without a GPU by
 * tests/test_tonebank_host.py.  Covers create over the corners of the supported
 * (C, F, B, hold) range with both windows, every rejected argument, the getters
 * and setters before any device work, the table design against the double
 * formula written here, num_outputs over the first blocks of a stream, every
 * argument error of execute (decided on the host), a well-formed execute (an
 * error without a device, a call with one), reset and destroy.
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

static double tones[65];

static void tables(ldsp_tonebank_t q, unsigned F, unsigned B, int window)
{
    const double two_pi = 2.0 * M_PI;
    float *tc = (float *)malloc((size_t)F * B * sizeof(float)), *ts = (float *)malloc((size_t)F * B * sizeof(float));
    double *f = (double *)malloc(F * sizeof(double)), *w = (double *)malloc(B * sizeof(double)), sumw = -1.0, sum = 0.0;
    CHECK(ldsp_tonebank_get_tables(q, f, tc, ts, &sumw) == LDSP_OK);
    CHECK(ldsp_tonebank_get_tables(q, NULL, NULL, NULL, NULL) == LDSP_OK);
    for (unsigned i = 0; i < B; i++) {
        w[i] = window == LDSP_TONE_HANN ? 0.5 - 0.5 * cos(two_pi * (double)i / (double)B) : 1.0;
        sum += w[i];
    }
    CHECK(sumw == sum);
    CHECK(fabs(sum - (window == LDSP_TONE_HANN ? 0.5 * B : 1.0 * B)) <= 1e-9 * B);
    const double s = sqrt(2.0) / sum;
    int bad = 0;
    for (unsigned k = 0; k < F; k++) {
        CHECK(f[k] == tones[k]);
        for (unsigned i = 0; i < B; i++) {
            const double ph = two_pi * tones[k] * (double)i;
            bad += tc[(size_t)k * B + i] != (float)(s * w[i] * cos(ph));
            bad += ts[(size_t)k * B + i] != (float)(-s * w[i] * sin(ph));
        }
    }
    CHECK(bad == 0);
    free(w);
    free(f);
    free(ts);
    free(tc);
}

static void shapes(void)
{
    const unsigned Cs[] = {1, 3, 256}, Fs[] = {2, 33, 64}, Bs[] = {64, 192, 16384}, Hs[] = {0, 1, 64};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            for (int l = 0; l < 3; l++) {
                const unsigned C = Cs[i], F = Fs[j], B = Bs[l], H = Hs[(i + j + l) % 3];
                const int window = (i + j + l) % 2 ? LDSP_TONE_HANN : LDSP_TONE_RECT;
                ldsp_tonebank_t q = NULL;
                CHECK(ldsp_tonebank_create(C, tones, F, B, window, 8.0, 0.0f, H, &q) == LDSP_OK && q != NULL);
                unsigned Co = 0, Fo = 0, Bo = 0, Ho = 99, fill = 99;
                int win = -1;
                CHECK(ldsp_tonebank_get_info(q, &Co, &Fo, &Bo, &win, &Ho, &fill) == LDSP_OK);
                CHECK(Co == C && Fo == F && Bo == B && win == window && Ho == H && fill == 0);
                CHECK(ldsp_tonebank_get_info(q, NULL, NULL, NULL, NULL, NULL, NULL) == LDSP_OK);
                if (i == 0) tables(q, F, B, window);
                int *want = (int *)malloc(C * sizeof(int)), *since = (int *)malloc(C * sizeof(int));
                CHECK(ldsp_tonebank_get_want(q, want) == LDSP_OK);
                for (unsigned c = 0; c < C; c++) CHECK(want[c] == -1);
                for (unsigned c = 0; c < C; c++) want[c] = (int)(c % F);
                CHECK(ldsp_tonebank_set_want(q, want, C) == LDSP_OK);
                memset(want, 0x55, C * sizeof(int));
                CHECK(ldsp_tonebank_get_want(q, want) == LDSP_OK);
                for (unsigned c = 0; c < C; c++) CHECK(want[c] == (int)(c % F));
                const int last = (int)F - 1, any = -1, over = (int)F, under = -2;
                CHECK(ldsp_tonebank_set_want(q, &last, 1) == LDSP_OK);
                CHECK(ldsp_tonebank_set_want(q, &any, 1) == LDSP_OK);
                CHECK(ldsp_tonebank_set_want(q, &over, 1) == LDSP_EINVAL);
                CHECK(ldsp_tonebank_set_want(q, &under, 1) == LDSP_EINVAL);
                CHECK(ldsp_tonebank_set_want(q, NULL, 1) == LDSP_EINVAL);
                if (C > 2) CHECK(ldsp_tonebank_set_want(q, want, 2) == LDSP_EINVAL);
                CHECK(ldsp_tonebank_set_want(q, want, 0) == LDSP_EINVAL);
                CHECK(ldsp_tonebank_get_want(q, want) == LDSP_OK);
                for (unsigned c = 0; c < C; c++) CHECK(want[c] == -1);
                CHECK(ldsp_tonebank_get_state(q, since) == LDSP_OK);
                for (unsigned c = 0; c < C; c++) CHECK(since[c] == 65);
                CHECK(ldsp_tonebank_get_state(q, NULL) == LDSP_EINVAL);
                size_t nb = 99;
                CHECK(ldsp_tonebank_num_outputs(q, 0, &nb) == LDSP_OK && nb == 0);
                CHECK(ldsp_tonebank_num_outputs(q, B - 1, &nb) == LDSP_OK && nb == 0);
                CHECK(ldsp_tonebank_num_outputs(q, B, &nb) == LDSP_OK && nb == 1);
                CHECK(ldsp_tonebank_num_outputs(q, 5 * (size_t)B + 3, &nb) == LDSP_OK && nb == 5);
                CHECK(ldsp_tonebank_num_outputs(q, 1, NULL) == LDSP_EINVAL);
                CHECK(ldsp_tonebank_reset(q) == LDSP_OK);
                CHECK(ldsp_tonebank_destroy(q) == LDSP_OK);
                free(since);
                free(want);
            }
}

static void rejected(void)
{
    ldsp_tonebank_t q = NULL;
    double bad[3] = {0.1, 0.2, 0.3};
    CHECK(ldsp_tonebank_create(0, tones, 3, 256, LDSP_TONE_HANN, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(257, tones, 3, 256, LDSP_TONE_HANN, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 1, 256, LDSP_TONE_HANN, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 0, 256, LDSP_TONE_HANN, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 65, 256, LDSP_TONE_HANN, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, NULL, 3, 256, LDSP_TONE_HANN, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    const double fs[] = {0.0, 0.5, -0.1, 0.7, NAN, INFINITY};
    for (int i = 0; i < 6; i++) {
        bad[1] = fs[i];
        CHECK(ldsp_tonebank_create(3, bad, 3, 256, LDSP_TONE_HANN, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    }
    const unsigned Bs[] = {0, 63, 100, 16448, 32768};
    for (int i = 0; i < 5; i++)
        CHECK(ldsp_tonebank_create(3, tones, 3, Bs[i], LDSP_TONE_HANN, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 3, 256, 2, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 3, 256, -1, 8.0, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 3, 256, LDSP_TONE_HANN, 0.99, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 3, 256, LDSP_TONE_HANN, NAN, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 3, 256, LDSP_TONE_HANN, INFINITY, 0.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 3, 256, LDSP_TONE_HANN, 8.0, -1.0f, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 3, 256, LDSP_TONE_HANN, 8.0, NAN, 1, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 3, 256, LDSP_TONE_HANN, 8.0, 0.0f, 65, &q) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_create(3, tones, 3, 256, LDSP_TONE_HANN, 8.0, 0.0f, 1, NULL) == LDSP_EINVAL);
    CHECK(q == NULL);
    CHECK(strlen(ldsp_last_error()) > 0);
    CHECK(ldsp_tonebank_reset(NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_get_info(NULL, NULL, NULL, NULL, NULL, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_get_tables(NULL, NULL, NULL, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_destroy(NULL) == LDSP_OK);
    size_t t = 0;
    CHECK(ldsp_debug_tonebank_tile(64, &t) == LDSP_OK && t >= 32 && t % 32 == 0);
    CHECK(ldsp_debug_tonebank_tile(16384, &t) == LDSP_OK && t >= 32 && t % 32 == 0);
    CHECK(ldsp_debug_tonebank_tile(100, &t) == LDSP_EINVAL);
    CHECK(ldsp_debug_tonebank_tile(64, NULL) == LDSP_EINVAL);
}

static void settings(void)
{
    ldsp_tonebank_t q = NULL;
    CHECK(ldsp_tonebank_create(2, tones, 5, 128, LDSP_TONE_RECT, 4.0, 0.25f, 3, &q) == LDSP_OK);
    double d = 0.0;
    float f = -1.0f;
    CHECK(ldsp_tonebank_get_dominance(q, &d) == LDSP_OK && d == 4.0);
    CHECK(ldsp_tonebank_get_floor(q, &f) == LDSP_OK && f == 0.25f);
    CHECK(ldsp_tonebank_set_dominance(q, 1.0) == LDSP_OK);
    CHECK(ldsp_tonebank_set_dominance(q, 0.5) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_set_dominance(q, NAN) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_get_dominance(q, &d) == LDSP_OK && d == 1.0);
    CHECK(ldsp_tonebank_set_floor(q, 0.0f) == LDSP_OK);
    CHECK(ldsp_tonebank_set_floor(q, -0.5f) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_set_floor(q, NAN) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_get_floor(q, &f) == LDSP_OK && f == 0.0f);
    CHECK(ldsp_tonebank_get_dominance(q, NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_get_floor(q, NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_destroy(q) == LDSP_OK);
}

static void execute(void)
{
    enum { C = 2, F = 5, B = 128, K = 3 * B + 7, N = 3 };
    ldsp_tonebank_t q = NULL;
    CHECK(ldsp_tonebank_create(C, tones, F, B, LDSP_TONE_HANN, 8.0, 0.0f, 1, &q) == LDSP_OK);
    float *x = (float *)calloc((size_t)C * K, sizeof(float)), *y = (float *)calloc((size_t)C * N * B, sizeof(float));
    float *pw = (float *)calloc((size_t)C * N * F, sizeof(float));
    int8_t tn[C * N];
    uint8_t op[C * N];
    size_t nb = 99;
    for (int i = 0; i < C * K; i++) x[i] = (float)sin(2.0 * M_PI * tones[i < K ? 1 : 3] * (double)(i % K));
    /* argument errors come before any device work and consume nothing */
    CHECK(ldsp_tonebank_execute(NULL, x, K, K, pw, N * F, tn, N, op, N, y, N * B, &nb, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_execute(q, x, K - 1, K, pw, N * F, tn, N, op, N, y, N * B, &nb, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_execute(q, NULL, K, K, pw, N * F, tn, N, op, N, y, N * B, &nb, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_execute(q, x, K, K, NULL, N * F, tn, N, op, N, y, N * B, &nb, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_execute(q, x, K, K, pw, N * F, NULL, N, op, N, y, N * B, &nb, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
    CHECK(ldsp_tonebank_execute(q, x, K, K, pw, N * F, tn, N, op, N, y, N * B, &nb, 7, NULL) == LDSP_EINVAL);
    nb = 99;
    CHECK(ldsp_tonebank_execute(q, x, K, K, pw, N * F - 1, tn, N, op, N, y, N * B, &nb, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
    CHECK(nb == N);
    CHECK(ldsp_tonebank_execute(q, x, K, K, pw, N * F, tn, N - 1, op, N, y, N * B, &nb, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
    CHECK(ldsp_tonebank_execute(q, x, K, K, pw, N * F, tn, N, op, N - 1, y, N * B, &nb, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
    CHECK(ldsp_tonebank_execute(q, x, K, K, pw, N * F, tn, N, op, N, y, N * B - 1, &nb, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
    unsigned fill = 99;
    CHECK(ldsp_tonebank_get_info(q, NULL, NULL, NULL, NULL, NULL, &fill) == LDSP_OK && fill == 0);
    /* a well-formed call: an error without a device, a block of a tone with one */
    const int rc = ldsp_tonebank_execute(q, x, K, K, pw, N * F, tn, N, op, N, y, N * B, &nb, LDSP_MEM_HOST, NULL);
    CHECK(rc == LDSP_OK || rc == LDSP_EHIP);
    CHECK(ldsp_tonebank_get_info(q, NULL, NULL, NULL, NULL, NULL, &fill) == LDSP_OK);
    if (rc == LDSP_OK) {
        CHECK(nb == N && fill == 7);
        for (int b = 0; b < N; b++) CHECK(tn[b] == 1 && tn[N + b] == 3 && op[b] == 1 && op[N + b] == 1);
        CHECK(fabsf(pw[1] - 0.5f) < 1e-3f);
        CHECK(memcmp(y, x, B * sizeof(float)) == 0);
        /* without open and without y */
        CHECK(ldsp_tonebank_execute(q, x, K, K, pw, N * F, tn, N, NULL, 0, y, N * B, &nb, LDSP_MEM_HOST, NULL) == LDSP_OK);
        CHECK(ldsp_tonebank_execute(q, x, K, K, pw, N * F, tn, N, NULL, 0, NULL, 0, &nb, LDSP_MEM_HOST, NULL) == LDSP_OK);
        int since[C];
        CHECK(ldsp_tonebank_get_state(q, since) == LDSP_OK && since[0] == 0 && since[1] == 0);
    } else {
        CHECK(fill == 0);
    }
    CHECK(ldsp_tonebank_reset(q) == LDSP_OK);
    CHECK(ldsp_tonebank_destroy(q) == LDSP_OK);
    free(pw);
    free(y);
    free(x);
}

int main(void)
{
    for (int k = 0; k < 65; k++) tones[k] = 0.01 + 0.007 * k;
    shapes();
    rejected();
    settings();
    execute();
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("tonebank driver: all checks passed\n");
    return 0;
}
