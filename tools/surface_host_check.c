/*
 * surface_host_check.c — the host side of "score a segmentation by surface distance" under the sanitizers: mbn_surface_envelope, mbn_surface_tile,
 * mbn_surface_scratch_bytes and mbn_surface_metrics over the cases the tests name and at the edges of their arguments, from a program of its own
 * (no Python, no GPU):
 *
 *   PKG=cnn-mobilenet-v1-implementation-on-aws-fpga-using-opencl_amd
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$PKG/host tools/surface_host_check.c \
 *       $PKG/host/mbn_surface.c -lm -o /tmp/surface_host_check && /tmp/surface_host_check
 *
 * Exit status 0 and "surface host check: ok" when every answer is the expected one and the sanitizers saw nothing.
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
    /* the envelope: the largest shape, each refusal, the caller's error first */
    EXPECT(mbn_surface_envelope(1, 21, 64, 1, 1, 1, 0) == MBN_OK);
    EXPECT(mbn_surface_envelope(4, MBN_CONFUSION_MAX_CLASSES, MBN_SURFACE_MAX_BINS, 65535, 16384, 32767, 1) == MBN_OK);
    EXPECT(mbn_surface_envelope(2, 21, 64, 1, 5, 5, 1) == MBN_EINVAL && mbn_surface_envelope(1, 0, 64, 1, 5, 5, 1) == MBN_EINVAL);
    EXPECT(mbn_surface_envelope(1, 21, 1, 1, 5, 5, 1) == MBN_EINVAL && mbn_surface_envelope(1, 21, 64, 0, 5, 5, 1) == MBN_EINVAL);
    EXPECT(mbn_surface_envelope(1, 21, 64, 1, -2147483647 - 1, 5, 1) == MBN_EINVAL && mbn_surface_envelope(1, 21, 64, 1, 5, 5, 2) == MBN_EINVAL);
    EXPECT(mbn_surface_envelope(1, MBN_CONFUSION_MAX_CLASSES + 1, 64, 1, 5, 5, 1) == MBN_EUNSUPPORTED);
    EXPECT(mbn_surface_envelope(1, 21, MBN_SURFACE_MAX_BINS + 1, 1, 5, 5, 1) == MBN_EUNSUPPORTED);
    EXPECT(mbn_surface_envelope(1, 21, 64, 1, 32768, 1, 1) == MBN_EUNSUPPORTED && mbn_surface_envelope(1, 21, 64, 1, 1, 2147483647, 1) == MBN_EUNSUPPORTED);
    EXPECT(mbn_surface_envelope(1, 21, 64, 1, 16385, 32767, 1) == MBN_EUNSUPPORTED && mbn_surface_envelope(1, 21, 64, 65536, 5, 5, 1) == MBN_EUNSUPPORTED);
    EXPECT(mbn_surface_envelope(1, 21, 64, 65536, 5, 5, 3) == MBN_EINVAL);
    int unit = 0, wave = 0;
    EXPECT(mbn_surface_tile(&unit, &wave) == MBN_OK && unit == MBN_SURFACE_UNIT && wave == 64 && unit % wave == 0);
    EXPECT(mbn_surface_tile(NULL, &wave) == MBN_EINVAL && mbn_surface_tile(&unit, NULL) == MBN_EINVAL);
    const int64_t big = (int64_t)1 << 34;
    EXPECT(mbn_surface_scratch_bytes(1, 1, 1) == 256 && mbn_surface_scratch_bytes(65535, big, MBN_CONFUSION_MAX_CLASSES) >= 8 * big);
    EXPECT(mbn_surface_scratch_bytes(0, 1, 1) == 0 && mbn_surface_scratch_bytes(1, 0, 1) == 0 && mbn_surface_scratch_bytes(1, 1, 0) == 0);
    EXPECT(mbn_surface_scratch_bytes(65536, 1, 1) == 0 && mbn_surface_scratch_bytes(1, big + 1, 1) == 0 && mbn_surface_scratch_bytes(2147483647, INT64_MAX, 2147483647) == 0);

    /* the metrics by hand (tests/test_surface_cpu.py, test_metrics_by_hand), from a heap table of exactly its size */
    const int bins = 4;
    const uint64_t cells[16] = { 10, 2, 10, 2000, 4, 2, 1, 1, 4, 0, 1, 1024, 0, 4, 0, 0 };
    uint64_t *surf = malloc(sizeof cells);
    double *per = malloc(4 * sizeof(double));
    EXPECT(surf && per);
    memcpy(surf, cells, sizeof cells);
    mbn_surface_metrics_t m;
    EXPECT(mbn_surface_metrics(surf, 1, bins, 1, 95.0, &m, per, per + 1, per + 2, per + 3) == MBN_OK);
    EXPECT(per[0] == sqrt(10.0) && per[1] == 3.0 && per[2] == 3024.0 / 256.0 / 12.0 && per[3] == 10.0 / 14.0);
    EXPECT(m.classes_present == 1 && m.classes_measurable == 1 && m.saturated == 1 && m.n == 14.0 && m.unmatched == 2.0 && m.reserved == 0);
    EXPECT(mbn_surface_metrics(surf, 1, bins, 0, 50.0, &m, NULL, NULL, NULL, NULL) == MBN_OK && m.hdp == 1.0 && m.saturated == 0 && m.nsd == 4.0 / 14.0);
    EXPECT(mbn_surface_metrics(surf, 1, bins, 2, 100.0, &m, NULL, per + 1, NULL, NULL) == MBN_OK && per[1] == 3.0);
    /* one side unmatched: present, not measurable */
    surf[8] = 4; surf[9] = 4; surf[13] = 0;
    EXPECT(mbn_surface_metrics(surf, 1, bins, 1, 95.0, &m, per, per + 1, per + 2, per + 3) == MBN_OK);
    EXPECT(isnan(per[0]) && isnan(per[1]) && isnan(per[2]) && per[3] == 6.0 / 14.0 && m.classes_present == 1 && m.classes_measurable == 0 && m.hd == 0.0);
    memset(surf, 0, sizeof cells);
    EXPECT(mbn_surface_metrics(surf, 1, bins, 1, 95.0, &m, per, per + 1, per + 2, per + 3) == MBN_OK && isnan(per[3]) && m.classes_present == 0 && m.nsd == 0.0);
    /* the same 16 cells as two classes of two bins: the last cell read is the table's last */
    EXPECT(mbn_surface_metrics(surf, 1, 2, 0, 95.0, &m, NULL, NULL, NULL, NULL) == MBN_OK);
    /* the refusals */
    EXPECT(mbn_surface_metrics(NULL, 1, bins, 1, 95.0, &m, NULL, NULL, NULL, NULL) == MBN_EINVAL && mbn_surface_metrics(surf, 1, bins, 1, 95.0, NULL, NULL, NULL, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_surface_metrics(surf, 0, bins, 1, 95.0, &m, NULL, NULL, NULL, NULL) == MBN_EINVAL && mbn_surface_metrics(surf, 1, 1, 0, 95.0, &m, NULL, NULL, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_surface_metrics(surf, 1, bins, -1, 95.0, &m, NULL, NULL, NULL, NULL) == MBN_EINVAL && mbn_surface_metrics(surf, 1, bins, 3, 95.0, &m, NULL, NULL, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_surface_metrics(surf, 1, bins, 1, 0.0, &m, NULL, NULL, NULL, NULL) == MBN_EINVAL && mbn_surface_metrics(surf, 1, bins, 1, 100.0000001, &m, NULL, NULL, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_surface_metrics(surf, 1, bins, 1, (double)NAN, &m, NULL, NULL, NULL, NULL) == MBN_EINVAL);
    EXPECT(mbn_surface_metrics(surf, MBN_CONFUSION_MAX_CLASSES + 1, bins, 1, 95.0, &m, NULL, NULL, NULL, NULL) == MBN_EUNSUPPORTED);
    EXPECT(mbn_surface_metrics(surf, 1, MBN_SURFACE_MAX_BINS + 1, 1, 95.0, &m, NULL, NULL, NULL, NULL) == MBN_EUNSUPPORTED);
    free(surf); free(per);
    printf("surface host check: ok\n");
    return 0;
}
