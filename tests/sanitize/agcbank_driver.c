/* Host-only exercise of the AGCBank's C ABI (ldsp_agcbank_*) under ASan / UBSan,
 * linked against the instrumented library of `make asan` and built by
 * `make -C python-liquiddsp_amd agcbank_asan`; run without a GPU by
 * tests/test_agcbank_host.py.  Covers create over the corners of the supported
 * (C, B, H) range for real and complex rows with one target and one per row,
 * every rejected argument, get_info / get_state before any device work, the dB
 * to unit conversion, num_outputs over the first blocks of a stream, every
 * argument error of execute (decided on the host), a well-formed execute (an
 * error without a device, a call with one), reset, destroy, and the partitioned
 * tracker of csrc/agc_track.hpp against the serial recurrence written here, for
 * several hangs, decays, partition widths and cuts of the stream.
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

#define AQ (1 << 24)
#define AFLOOR (-64 * AQ)
#define ACEIL (64 * AQ)

static double targets[257];

static void shapes(void)
{
    const unsigned Cs[] = {1, 3, 256}, Bs[] = {16, 100, 4096}, Hs[] = {0, 8, 255};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            for (int l = 0; l < 3; l++)
                for (int cx = 0; cx < 2; cx++) {
                    const unsigned C = Cs[i], B = Bs[j], H = Hs[l];
                    const unsigned nt = (i + j + l) % 2 ? C : 1;
                    ldsp_agcbank_t q = NULL;
                    CHECK(ldsp_agcbank_create(C, B, targets, nt, 60.0, H, 0.5, cx, &q) == LDSP_OK && q != NULL);
                    unsigned Co = 0, Bo = 0, Ho = 99, fill = 99;
                    int cplx = -1;
                    double dec = -1.0, mg = -1.0;
                    double *t = (double *)malloc(C * sizeof(double));
                    CHECK(ldsp_agcbank_get_info(q, &Co, &Bo, &Ho, &dec, &mg, t, &cplx, &fill) == LDSP_OK);
                    CHECK(Co == C && Bo == B && Ho == H && dec == 0.5 && mg == 60.0 && cplx == cx && fill == 0);
                    for (unsigned c = 0; c < C; c++) CHECK(t[c] == targets[nt == 1 ? 0 : c]);
                    CHECK(ldsp_agcbank_get_info(q, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == LDSP_OK);
                    int32_t *lv = (int32_t *)malloc(C * sizeof(int32_t));
                    int32_t *pk = (int32_t *)malloc((size_t)C * (H ? H : 1) * sizeof(int32_t));
                    float *gn = (float *)malloc((size_t)C * 2 * sizeof(float));
                    CHECK(ldsp_agcbank_get_state(q, lv, pk, gn) == LDSP_OK);
                    for (unsigned c = 0; c < C; c++) CHECK(lv[c] == AFLOOR && gn[2 * c] == 0.0f && gn[2 * c + 1] == 0.0f);
                    for (size_t k = 0; k < (size_t)C * H; k++) CHECK(pk[k] == AFLOOR);
                    CHECK(ldsp_agcbank_get_state(q, NULL, NULL, NULL) == LDSP_OK);
                    size_t tr = 99, em = 99;
                    CHECK(ldsp_agcbank_num_outputs(q, 0, &tr, &em) == LDSP_OK && tr == 0 && em == 0);
                    CHECK(ldsp_agcbank_num_outputs(q, B - 1, &tr, &em) == LDSP_OK && tr == 0 && em == 0);
                    CHECK(ldsp_agcbank_num_outputs(q, B, &tr, &em) == LDSP_OK && tr == 1 && em == 0);
                    CHECK(ldsp_agcbank_num_outputs(q, 2 * B, &tr, &em) == LDSP_OK && tr == 2 && em == 1);
                    CHECK(ldsp_agcbank_num_outputs(q, 5 * B + 3, &tr, NULL) == LDSP_OK && tr == 5);
                    CHECK(ldsp_agcbank_num_outputs(q, 5 * B + 3, NULL, &em) == LDSP_OK && em == 4);
                    CHECK(ldsp_agcbank_num_outputs(q, 1, NULL, NULL) == LDSP_EINVAL);
                    CHECK(ldsp_agcbank_reset(q) == LDSP_OK);
                    CHECK(ldsp_agcbank_destroy(q) == LDSP_OK);
                    free(gn);
                    free(pk);
                    free(lv);
                    free(t);
                }
}

static void rejected(void)
{
    ldsp_agcbank_t q = NULL;
    const double one = -12.0, bad_nan = NAN, bad_big = 200.0;
    CHECK(ldsp_agcbank_create(0, 256, &one, 1, 60.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(257, 256, targets, 1, 60.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 15, &one, 1, 60.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 4097, &one, 1, 60.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, &one, 1, 60.0, 256, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, &one, 1, 60.0, 8, -0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, &one, 1, 60.0, 8, NAN, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, &one, 1, NAN, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, &one, 1, 181.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, &bad_nan, 1, 60.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, &bad_big, 1, 60.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, targets, 2, 60.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, targets, 0, 60.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, NULL, 1, 60.0, 8, 0.5, 0, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, &one, 1, 60.0, 8, 0.5, 2, &q) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_create(3, 256, &one, 1, 60.0, 8, 0.5, 0, NULL) == LDSP_EINVAL);
    CHECK(q == NULL);
    CHECK(strlen(ldsp_last_error()) > 0);
    CHECK(ldsp_agcbank_reset(NULL) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_get_info(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_get_state(NULL, NULL, NULL, NULL) == LDSP_EINVAL);
    CHECK(ldsp_agcbank_destroy(NULL) == LDSP_OK);
}

static void units(void)
{
    int64_t u = 0;
    CHECK(ldsp_debug_agcbank_units(0.0, &u) == LDSP_OK && u == 0);
    CHECK(ldsp_debug_agcbank_units(20.0 * log10(2.0), &u) == LDSP_OK && u == AQ);
    CHECK(ldsp_debug_agcbank_units(-40.0 * log10(2.0), &u) == LDSP_OK && u == -2 * AQ);
    CHECK(ldsp_debug_agcbank_units(0.5, &u) == LDSP_OK && u == llrint(0.5 * 16777216.0 / (20.0 * log10(2.0))));
    CHECK(ldsp_debug_agcbank_units(1.0e9, &u) == LDSP_OK && u > 0);
    CHECK(ldsp_debug_agcbank_units(NAN, &u) == LDSP_EINVAL);
    CHECK(ldsp_debug_agcbank_units(INFINITY, &u) == LDSP_EINVAL);
    CHECK(ldsp_debug_agcbank_units(1.0, NULL) == LDSP_EINVAL);
}

static void execute_paths(void)
{
    for (int cx = 0; cx < 2; cx++) {
        ldsp_agcbank_t q = NULL;
        const double one = -12.0;
        CHECK(ldsp_agcbank_create(3, 16, &one, 1, 60.0, 2, 0.5, cx, &q) == LDSP_OK);
        const size_t es = cx ? 2 : 1;
        float *x = (float *)calloc(3 * 64 * es, sizeof(float));
        float *y = (float *)calloc(3 * 48 * es, sizeof(float));
        int32_t pq[12], gq[12];
        size_t nw = 0;
        for (size_t i = 0; i < 3 * 64 * es; i++) x[i] = 0.25f;
        CHECK(ldsp_agcbank_execute(q, x, 64, 64, y, 47, pq, gq, 4, &nw, LDSP_MEM_HOST, NULL) == LDSP_ERANGE && nw == 48);
        CHECK(ldsp_agcbank_execute(q, x, 64, 64, y, 48, pq, gq, 3, &nw, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
        CHECK(ldsp_agcbank_execute(q, x, 64, 64, y, 47, pq, gq, 4, NULL, LDSP_MEM_HOST, NULL) == LDSP_ERANGE);
        CHECK(ldsp_agcbank_execute(q, x, 63, 64, y, 48, pq, gq, 4, &nw, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
        CHECK(ldsp_agcbank_execute(NULL, x, 64, 64, y, 48, pq, gq, 4, &nw, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
        CHECK(ldsp_agcbank_execute(q, NULL, 64, 64, y, 48, pq, gq, 4, &nw, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
        CHECK(ldsp_agcbank_execute(q, x, 64, 64, NULL, 48, pq, gq, 4, &nw, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
        CHECK(ldsp_agcbank_execute(q, x, 64, 64, y, 48, NULL, gq, 4, &nw, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
        CHECK(ldsp_agcbank_execute(q, x, 64, 64, y, 48, pq, NULL, 4, &nw, LDSP_MEM_HOST, NULL) == LDSP_EINVAL);
        CHECK(ldsp_agcbank_execute(q, x, 64, 64, y, 48, pq, gq, 4, &nw, 7, NULL) == LDSP_EINVAL);
        unsigned fill = 99;
        CHECK(ldsp_agcbank_get_info(q, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &fill) == LDSP_OK && fill == 0);
        /* a well-formed call: an error without a device (no fallback), a result with one */
        const int rc = ldsp_agcbank_execute(q, x, 64, 64, y, 48, pq, gq, 4, &nw, LDSP_MEM_HOST, NULL);
        CHECK(rc == LDSP_EHIP || rc == LDSP_OK);
        CHECK(ldsp_agcbank_get_info(q, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &fill) == LDSP_OK);
        CHECK(fill == (rc == LDSP_OK ? 16u : 0u));
        if (rc == LDSP_OK)
            for (size_t i = 0; i < 3 * 48 * es; i++) CHECK(fabsf(y[i]) <= 0.2512f);
        CHECK(ldsp_agcbank_reset(q) == LDSP_OK);
        CHECK(ldsp_agcbank_get_info(q, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &fill) == LDSP_OK && fill == 0);
        CHECK(ldsp_agcbank_destroy(q) == LDSP_OK);
        free(y);
        free(x);
    }
}

/* L_b = max(w_b, L_{b-1} - d, FLOOR), w_b = max(p[b - H .. b]), written out */
static void serial(const int32_t *p, size_t n, unsigned H, int64_t d, int32_t *L)
{
    int64_t cur = AFLOOR;
    for (size_t b = 0; b < n; b++) {
        int64_t w = AFLOOR;
        for (size_t j = b >= H ? b - H : 0; j <= b; j++)
            if (p[j] > w) w = p[j];
        cur -= d;
        if (cur < w) cur = w;
        if (cur < AFLOOR) cur = AFLOOR;
        L[b] = (int32_t)cur;
    }
}

static uint32_t lcg = 12345u;
static uint32_t rnd(void)
{
    lcg = lcg * 1664525u + 1013904223u;
    return lcg >> 8;
}

static void tracker(void)
{
    enum { N = 1500 };
    const unsigned Hs[] = {0, 1, 7, 255};
    const int64_t ds[] = {0, 1, 1391979, 83518727, (int64_t)1 << 31};
    const size_t widths[] = {1, 3, 64, 257, 5000};
    int32_t *p = (int32_t *)malloc(N * sizeof(int32_t));
    int32_t *want = (int32_t *)malloc(N * sizeof(int32_t));
    int32_t *got = (int32_t *)malloc(N * sizeof(int32_t));
    for (int kind = 0; kind < 2; kind++) {
        for (size_t i = 0; i < N; i++)
            p[i] = kind == 0 ? (i == 0 ? ACEIL : AFLOOR) : (int32_t)((rnd() % 40u) * AQ + rnd() % AQ) - 38 * AQ;
        for (int h = 0; h < 4; h++)
            for (int k = 0; k < 5; k++) {
                serial(p, N, Hs[h], ds[k], want);
                for (int w = 0; w < 5; w++) {
                    int32_t level = AFLOOR, tail[255];
                    for (int i = 0; i < 255; i++) tail[i] = AFLOOR;
                    size_t at = 0;
                    while (at < N) {                     /* ragged calls, empty ones among them */
                        size_t len = rnd() % 400;
                        if (len > N - at) len = N - at;
                        CHECK(ldsp_debug_agcbank_track(p + at, len, Hs[h], ds[k], widths[w], &level, Hs[h] ? tail : NULL,
                                                       got + at) == LDSP_OK);
                        at += len;
                    }
                    CHECK(memcmp(got, want, N * sizeof(int32_t)) == 0);
                    CHECK(level == want[N - 1]);
                    for (unsigned i = 0; i < Hs[h]; i++) CHECK(tail[i] == p[N - Hs[h] + i]);
                }
            }
    }
    int32_t level = AFLOOR, tail[4] = {AFLOOR, AFLOOR, AFLOOR, AFLOOR};
    CHECK(ldsp_debug_agcbank_track(NULL, 8, 4, 5, 3, &level, tail, got) == LDSP_EINVAL);
    CHECK(ldsp_debug_agcbank_track(p, 8, 4, 5, 3, &level, tail, NULL) == LDSP_EINVAL);
    CHECK(ldsp_debug_agcbank_track(p, 8, 4, 5, 3, NULL, tail, got) == LDSP_EINVAL);
    CHECK(ldsp_debug_agcbank_track(p, 8, 4, 5, 3, &level, NULL, got) == LDSP_EINVAL);
    CHECK(ldsp_debug_agcbank_track(p, 8, 256, 5, 3, &level, tail, got) == LDSP_EINVAL);
    CHECK(ldsp_debug_agcbank_track(p, 8, 4, -1, 3, &level, tail, got) == LDSP_EINVAL);
    CHECK(ldsp_debug_agcbank_track(p, 8, 4, 5, 0, &level, tail, got) == LDSP_EINVAL);
    p[3] = ACEIL + 1;
    CHECK(ldsp_debug_agcbank_track(p, 8, 4, 5, 3, &level, tail, got) == LDSP_EINVAL);
    CHECK(ldsp_debug_agcbank_track(NULL, 0, 0, 5, 3, &level, NULL, NULL) == LDSP_OK);
    free(got);
    free(want);
    free(p);
}

int main(void)
{
    for (int c = 0; c < 257; c++) targets[c] = -30.0 + (double)c / 8.0;
    shapes();
    rejected();
    units();
    execute_paths();
    tracker();
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
