/*
 * nll_host_check.c — the host side of "score the probabilities" under the sanitizers: mbn_nll_metrics, mbn_nll_best, mbn_resample_nll_envelope,
 * mbn_resample_nll_ragged_check and mbn_nll_temps_check at the edges of their arguments, on heap tables of exactly their size, from a program
 * of its own (no Python, no GPU):
 *
 *   PKG=cnn-mobilenet-v1-implementation-on-aws-fpga-using-opencl_amd
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$PKG/host tools/nll_host_check.c \
 *       $PKG/host/mbn_score.c $PKG/host/mbn_envelope.c -lm -o /tmp/nll_host_check && /tmp/nll_host_check
 *
 * Exit status 0 and "nll host check: ok" when every answer is the expected one and the sanitizers saw nothing.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mbn.h"
#include "mbn_envelope.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

/* a heap table [temps][classes + 1][4] of exactly its size, zeroed */
static uint64_t *table(int classes, int temps) { return calloc((size_t)temps * ((size_t)classes + 1) * 4, sizeof(uint64_t)); }

int main(void)
{
    /* the envelope: the largest arguments, each refusal, the caller's error first */
    const int32_t full[4] = { 0, 0, 64, 64 }, off[4] = { 1, 0, 64, 64 };
    EXPECT(mbn_resample_nll_envelope(1, 2, 2, 21, 0, 0, NULL, 16, 16, 1, 1) == MBN_OK);
    EXPECT(mbn_resample_nll_envelope(65535, 2, 2, MBN_CONFUSION_MAX_CLASSES, 64, 64, full, 16, 16, 4, MBN_NLL_MAX_TEMPS) == MBN_OK);
    EXPECT(mbn_resample_nll_envelope(1, 2, 2, 21, 0, 0, NULL, 16, 16, 2, 1) == MBN_EINVAL && mbn_resample_nll_envelope(1, 2, 2, 21, 0, 0, NULL, 16, 16, 1, 0) == MBN_EINVAL);
    EXPECT(mbn_resample_nll_envelope(1, 2, 2, 21, 0, 0, NULL, 16, 16, 1, MBN_NLL_MAX_TEMPS + 1) == MBN_EINVAL);
    EXPECT(mbn_resample_nll_envelope(1, 2, 2, 21, 0, 0, NULL, 16, 16, 1, -2147483647 - 1) == MBN_EINVAL);
    EXPECT(mbn_resample_nll_envelope(0, 2, 2, 21, 0, 0, NULL, 16, 16, 1, 1) == MBN_EINVAL && mbn_resample_nll_envelope(1, 2, 2, 21, 64, 64, off, 16, 16, 1, 1) == MBN_EINVAL);
    EXPECT(mbn_resample_nll_envelope(1, 2, 2, MBN_CONFUSION_MAX_CLASSES + 1, 0, 0, NULL, 16, 16, 1, 1) == MBN_EUNSUPPORTED);
    EXPECT(mbn_resample_nll_envelope(1, 2, 2, 21, 0, 0, NULL, 7, 16, 1, 1) == MBN_EUNSUPPORTED && mbn_resample_nll_envelope(65536, 2, 2, 21, 0, 0, NULL, 16, 16, 1, 1) == MBN_EUNSUPPORTED);
    EXPECT(mbn_resample_nll_envelope(1, 2, 2, 21, 0, 0, NULL, 7, 16, 3, 1) == MBN_EINVAL && mbn_resample_nll_envelope(1, 2, 2, 2147483647, 0, 0, NULL, 16, 16, 1, 9) == MBN_EINVAL);
    EXPECT(mbn_resample_nll_envelope(65535, 4096, 4096, 21, 0, 0, NULL, 16384, 16384, 1, 8) == MBN_EUNSUPPORTED);
    EXPECT(mbn_resample_nll_ragged_check(21, 100, 1, 3, 100) == MBN_OK && mbn_resample_nll_ragged_check(21, 100, 4, 8, MBN_TOPK_MAX_ELEMENTS / 8) == MBN_OK);
    EXPECT(mbn_resample_nll_ragged_check(21, 100, 1, 3, 99) == MBN_EINVAL && mbn_resample_nll_ragged_check(0, 100, 1, 3, 100) == MBN_EINVAL);
    EXPECT(mbn_resample_nll_ragged_check(21, 0, 1, 3, 100) == MBN_EINVAL && mbn_resample_nll_ragged_check(21, 100, 3, 3, 100) == MBN_EINVAL);
    EXPECT(mbn_resample_nll_ragged_check(21, 100, 1, 8, MBN_TOPK_MAX_ELEMENTS / 8 + 1) == MBN_EUNSUPPORTED);
    EXPECT(mbn_resample_nll_ragged_check(21, 100, 1, 8, INT64_MAX) == MBN_EUNSUPPORTED && mbn_resample_nll_ragged_check(5000, 100, 1, 8, 100) == MBN_EUNSUPPORTED);

    /* the temperatures: the closed range [1/16, 16], one entry on the heap and eight */
    float *beta = malloc(MBN_NLL_MAX_TEMPS * sizeof(float));
    EXPECT(beta);
    for (int j = 0; j < MBN_NLL_MAX_TEMPS; j++) beta[j] = 0.0625f * (float)(1 << j) * (j == 7 ? 2.0f : 1.0f);      /* 1/16 .. 4, 16 */
    EXPECT(mbn_nll_temps_check(beta, MBN_NLL_MAX_TEMPS) == MBN_OK && mbn_nll_temps_check(beta + 7, 1) == MBN_OK);
    EXPECT(mbn_nll_temps_check(NULL, 1) == MBN_EINVAL && mbn_nll_temps_check(beta, 0) == MBN_EINVAL && mbn_nll_temps_check(beta, 9) == MBN_EINVAL);
    const float bad[6] = { nextafterf(0.0625f, 0.0f), nextafterf(16.0f, 17.0f), NAN, INFINITY, -1.0f, 0.0f };
    for (int i = 0; i < 6; i++) {
        beta[3] = bad[i];
        EXPECT(mbn_nll_temps_check(beta, MBN_NLL_MAX_TEMPS) == MBN_EINVAL && mbn_nll_temps_check(beta, 3) == MBN_OK);
    }
    beta[3] = 0.5f;

    /* the metrics by hand: 3 classes, 2 temperatures, class 1 absent */
    const int classes = 3, temps = 2;
    uint64_t *t = table(classes, temps);
    double *per = malloc(2 * (size_t)classes * sizeof(double));
    EXPECT(t && per);
    uint64_t *p1 = t + (size_t)(classes + 1) * 4;                  /* plane 1 */
    p1[0] = 4; p1[1] = 6 << 16; p1[2] = 2 << 24; p1[3] = 3;         /* class 0: 4 pixels, nll 1.5, brier 0.5, 3 right */
    p1[8] = 1; p1[9] = 1 << 15; p1[10] = 1 << 22; p1[11] = 0;       /* class 2: 1 pixel, nll 0.5, brier 0.25 */
    p1[12] = 7;                                                     /* void */
    mbn_nll m;
    EXPECT(mbn_nll_metrics(t, classes, temps, 1, &m, per, per + classes) == MBN_OK);
    EXPECT(m.scored == 5.0 && m.void_pixels == 7.0 && m.pixels == 12.0 && m.nll == 6.5 / 5.0 && m.brier == 2.25 / 5.0 && m.accuracy == 0.6);
    EXPECT(m.classes_present == 2 && m.mean_class_nll == 1.0 && m.mean_class_brier == 0.375);
    EXPECT(per[0] == 1.5 && isnan(per[1]) && per[2] == 0.5 && per[3] == 0.5 && isnan(per[4]) && per[5] == 0.25);
    EXPECT(mbn_nll_metrics(t, classes, temps, 0, &m, NULL, NULL) == MBN_OK && m.scored == 0.0 && m.nll == 0.0 && m.accuracy == 0.0 && m.classes_present == 0);
    EXPECT(mbn_nll_metrics(t, classes, temps, 2, &m, NULL, NULL) == MBN_EINVAL && mbn_nll_metrics(t, classes, temps, -1, &m, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_nll_metrics(NULL, classes, temps, 0, &m, NULL, NULL) == MBN_EINVAL && mbn_nll_metrics(t, classes, temps, 0, NULL, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_nll_metrics(t, 0, temps, 0, &m, NULL, NULL) == MBN_EINVAL && mbn_nll_metrics(t, classes, 9, 0, &m, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_nll_metrics(t, MBN_CONFUSION_MAX_CLASSES + 1, temps, 0, &m, NULL, NULL) == MBN_EUNSUPPORTED);
    /* cells near 2^63: the sums stay finite */
    p1[1] = (uint64_t)1 << 63;
    EXPECT(mbn_nll_metrics(t, classes, temps, 1, &m, NULL, NULL) == MBN_OK && isfinite(m.nll) && m.nll > 0.0);
    free(t);

    /* the best plane: the largest class count and eight temperatures on the heap; interior, both edges, a tie, nothing scored */
    const int big = MBN_CONFUSION_MAX_CLASSES;
    t = table(big, MBN_NLL_MAX_TEMPS);
    EXPECT(t);
    const double y[8] = { 5, 4, 3, 2.5, 2.75, 4, 5, 6 };
    for (int j = 0; j < 8; j++) {
        uint64_t *row = t + ((size_t)j * ((size_t)big + 1) + (size_t)(big - 1)) * 4;       /* the last class row */
        row[0] = 10; row[1] = (uint64_t)(y[j] * 65536.0) * 10;
    }
    int best = -1, edge = -1;
    double refined = 0.0;
    EXPECT(mbn_nll_best(t, big, 8, beta, &best, &refined, &edge) == MBN_OK && best == 3 && edge == 0);
    EXPECT(refined > (double)beta[2] && refined < (double)beta[4] && refined != (double)beta[3]);
    EXPECT(mbn_nll_best(t, big, 3, beta, &best, &refined, &edge) == MBN_OK && best == 2 && edge == 1 && refined == (double)beta[2]);
    EXPECT(mbn_nll_best(t + ((size_t)big + 1) * 4 * 3, big, 5, beta + 3, &best, NULL, NULL) == MBN_OK && best == 0);
    EXPECT(mbn_nll_best(t, big, 1, beta, &best, &refined, &edge) == MBN_OK && best == 0 && edge == 0);
    t[((size_t)4 * ((size_t)big + 1) + (size_t)(big - 1)) * 4 + 1] = t[((size_t)3 * ((size_t)big + 1) + (size_t)(big - 1)) * 4 + 1];
    EXPECT(mbn_nll_best(t, big, 8, beta, &best, &refined, &edge) == MBN_OK && best == 3);      /* a tie: the lowest index */
    beta[5] = beta[4];
    best = -7;
    EXPECT(mbn_nll_best(t, big, 8, beta, &best, &refined, &edge) == MBN_EINVAL && best == -7);
    beta[5] = 2.0f;
    EXPECT(mbn_nll_best(t, big, 8, NULL, &best, NULL, NULL) == MBN_EINVAL && mbn_nll_best(t, big, 8, beta, NULL, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_nll_best(NULL, big, 8, beta, &best, NULL, NULL) == MBN_EINVAL && mbn_nll_best(t, big, 0, beta, &best, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_nll_best(t, big + 1, 8, beta, &best, NULL, NULL) == MBN_EUNSUPPORTED);
    t[(size_t)(big - 1) * 4] = 0;                                   /* plane 0 scores nothing */
    EXPECT(mbn_nll_best(t, big, 8, beta, &best, &refined, &edge) == MBN_ENOTFOUND && best == -7);
    free(t);
    free(per);
    free(beta);
    puts("nll host check: ok");
    return 0;
}
