/*
 * confusion_host_check.c — the host side of "score a segmentation" under the sanitizers: mbn_confusion_metrics, mbn_confusion_form and
 * mbn_confusion_envelope over the cases the tests name, from a program of its own (no Python, no GPU):
 *
 *   PKG=cnn-mobilenet-v1-implementation-on-aws-fpga-using-opencl_amd
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$PKG/host tools/confusion_host_check.c \
 *       $PKG/host/mbn_score.c -lm -o /tmp/confusion_host_check && /tmp/confusion_host_check
 *
 * Exit status 0 and "confusion host check: ok" when every answer is the expected one and the sanitizers saw nothing.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mbn.h"
#include "mbn_envelope.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main(void)
{
    /* the known answer; counts and iou on the heap, exactly as large as the call may touch */
    {
        const uint64_t known[9] = { 5, 1, 2, 3, 4, 0, 7, 1, 1 };
        uint64_t *n = malloc(sizeof known);
        double *iou = malloc(2 * sizeof(double));
        EXPECT(n && iou);
        memcpy(n, known, sizeof known);
        mbn_seg_metrics m;
        memset(&m, 0xAB, sizeof m);
        EXPECT(mbn_confusion_metrics(n, 2, &m, iou) == MBN_OK);
        EXPECT(m.pixels == 24.0 && m.valid == 15.0 && m.void_pixels == 9.0 && m.abstained == 2.0 && m.classes_present == 2 && m.reserved == 0);
        EXPECT(m.pixel_accuracy == 9.0 / 15.0 && iou[0] == 5.0 / 11.0 && iou[1] == 4.0 / 8.0);
        EXPECT(m.miou == (5.0 / 11.0 + 1.0 / 2.0) / 2.0 && m.mean_accuracy == (5.0 / 8.0 + 4.0 / 7.0) / 2.0);
        EXPECT(m.fw_iou == (8.0 / 15.0) * (5.0 / 11.0) + (7.0 / 15.0) * (1.0 / 2.0));
        EXPECT(mbn_confusion_metrics(n, 2, &m, NULL) == MBN_OK && m.miou == (5.0 / 11.0 + 1.0 / 2.0) / 2.0);
        free(n); free(iou);
    }
    /* every class count's table read to its last cell and no further: 1, the last LDS count and its neighbour, the largest */
    const int sizes[] = { 1, 2, 21, MBN_CONFUSION_LDS_CLASSES, MBN_CONFUSION_LDS_CLASSES + 1, 1000, MBN_CONFUSION_MAX_CLASSES };
    for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; k++) {
        const int c = sizes[k];
        const size_t s = (size_t)c + 1;
        uint64_t *n = malloc(s * s * sizeof(uint64_t));
        double *iou = malloc((size_t)c * sizeof(double));
        EXPECT(n && iou);
        for (size_t i = 0; i < s * s; i++) n[i] = (i * 2654435761u) % 1000u;
        for (size_t i = 0; i < s; i++) n[i * s + i] += 5000u;
        mbn_seg_metrics m;
        EXPECT(mbn_confusion_metrics(n, c, &m, iou) == MBN_OK);
        double total = 0.0;
        for (size_t i = 0; i < s * s; i++) total += (double)n[i];
        EXPECT(m.pixels == total && m.valid + m.void_pixels == total && m.classes_present == c);
        EXPECT(m.miou > 0.0 && m.miou <= 1.0 && m.pixel_accuracy > 0.0 && m.pixel_accuracy <= 1.0 && m.fw_iou > 0.0 && m.fw_iou <= 1.0);
        for (int i = 0; i < c; i++) EXPECT(iou[i] > 0.0 && iou[i] <= 1.0);
        memset(n, 0, s * s * sizeof(uint64_t));                     /* nothing scored: no division by zero, every iou NaN */
        EXPECT(mbn_confusion_metrics(n, c, &m, iou) == MBN_OK);
        EXPECT(m.pixels == 0.0 && m.miou == 0.0 && m.mean_accuracy == 0.0 && m.fw_iou == 0.0 && m.pixel_accuracy == 0.0 && m.classes_present == 0);
        for (int i = 0; i < c; i++) EXPECT(isnan(iou[i]));
        n[s * s - 1] = UINT64_MAX;                                  /* the largest cell, in the void row: converted, never indexed with */
        EXPECT(mbn_confusion_metrics(n, c, &m, iou) == MBN_OK && m.valid == 0.0 && m.void_pixels == 18446744073709551616.0);
        free(n); free(iou);
    }
    /* the refusals */
    uint64_t one[4] = { 1, 0, 0, 0 };
    mbn_seg_metrics m;
    EXPECT(mbn_confusion_metrics(NULL, 1, &m, NULL) == MBN_EINVAL && mbn_confusion_metrics(one, 1, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_confusion_metrics(one, 0, &m, NULL) == MBN_EINVAL && mbn_confusion_metrics(one, -2147483647 - 1, &m, NULL) == MBN_EINVAL);
    EXPECT(mbn_confusion_metrics(one, MBN_CONFUSION_MAX_CLASSES + 1, &m, NULL) == MBN_EUNSUPPORTED);
    EXPECT(mbn_confusion_metrics(one, 2147483647, &m, NULL) == MBN_EUNSUPPORTED);
    /* the form: monotone, one switch point, over every int the predicate can be asked */
    int switches = 0;
    for (int c = 1; c <= MBN_CONFUSION_MAX_CLASSES; c++) {
        const int f = mbn_confusion_form(c);
        EXPECT(f == MBN_CONFUSION_FORM_LDS || f == MBN_CONFUSION_FORM_GLOBAL);
        if (c > 1 && f != mbn_confusion_form(c - 1)) { switches++; EXPECT(f == MBN_CONFUSION_FORM_GLOBAL && c == MBN_CONFUSION_LDS_CLASSES + 1); }
        if (f == MBN_CONFUSION_FORM_LDS) EXPECT((c + 1) * (c + 1) * 4 <= MBN_CONFUSION_LDS);
    }
    EXPECT(switches == 1 && mbn_confusion_form(21) == MBN_CONFUSION_FORM_LDS && mbn_confusion_form(1000) == MBN_CONFUSION_FORM_GLOBAL);
    EXPECT(mbn_confusion_form(-2147483647 - 1) == MBN_CONFUSION_FORM_LDS && mbn_confusion_form(2147483647) == MBN_CONFUSION_FORM_GLOBAL);
    /* the envelope: every status, the extreme arguments among them */
    EXPECT(mbn_confusion_envelope(21, 1, 1) == MBN_OK && mbn_confusion_envelope(MBN_CONFUSION_MAX_CLASSES, 4, MBN_CONFUSION_MAX_COUNT) == MBN_OK);
    EXPECT(mbn_confusion_envelope(0, 1, 1) == MBN_EINVAL && mbn_confusion_envelope(21, 1, 0) == MBN_EINVAL);
    EXPECT(mbn_confusion_envelope(21, 2, 1) == MBN_EINVAL && mbn_confusion_envelope(21, 0, 1) == MBN_EINVAL);
    EXPECT(mbn_confusion_envelope(-2147483647 - 1, 1, 1) == MBN_EINVAL && mbn_confusion_envelope(21, 1, INT64_MIN) == MBN_EINVAL);
    EXPECT(mbn_confusion_envelope(MBN_CONFUSION_MAX_CLASSES + 1, 1, 1) == MBN_EUNSUPPORTED);
    EXPECT(mbn_confusion_envelope(21, 4, MBN_CONFUSION_MAX_COUNT + 1) == MBN_EUNSUPPORTED && mbn_confusion_envelope(2147483647, 4, INT64_MAX) == MBN_EUNSUPPORTED);
    printf("confusion host check: ok\n");
    return 0;
}
