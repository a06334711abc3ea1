/*
 * ensemble_host_check.c — the host side of the ensemble read-out under the sanitizers: mbn_fit_view, mbn_resample_ensemble_envelope and
 * mbn_resample_ensemble_plan, once each over the cases the tests name, from a program of its own (no Python, no GPU):
 *
 *   PKG=cnn-mobilenet-v1-implementation-on-aws-fpga-using-opencl_amd
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$PKG/host tools/ensemble_host_check.c \
 *       $PKG/host/mbn_envelope.c $PKG/host/mbn_resize.c -lm -o /tmp/ensemble_host_check && /tmp/ensemble_host_check
 *
 * Exit status 0 and "ensemble host check: ok" when every answer is the expected one and the sanitizers saw nothing.
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
    /* views on the heap, exactly as many as are handed over: a read past the last one is the sanitizer's to find */
    for (int n = 1; n <= MBN_ENSEMBLE_MAX_VIEWS; n++) {
        mbn_view *v = malloc(sizeof(mbn_view) * (size_t)n);
        EXPECT(v != NULL);
        for (int k = 0; k < n; k++) {
            const float scale = 1.0f - 0.1f * (float)k;
            EXPECT(mbn_fit_view(375, 500, 224, 224, scale, k & 1, &v[k]) == MBN_OK);
            EXPECT(v[k].x >= 0 && v[k].y >= 0 && v[k].x + v[k].iw <= 224 && v[k].y + v[k].ih <= 224 && v[k].mirror == (k & 1));
            EXPECT(v[k].reserved[0] == 0 && v[k].reserved[1] == 0 && v[k].reserved[2] == 0);
        }
        EXPECT(mbn_resample_ensemble_envelope(32, 28, 28, 1000, 224, 224, v, n, 375, 500) == MBN_OK);
        mbn_resample_launch_t l;
        memset(&l, 0xAB, sizeof l);
        EXPECT(mbn_resample_ensemble_plan(28, 28, 224, 224, v, n, 375, 500, &l) == MBN_OK);
        EXPECT(l.fy >= 1 && l.fy <= 10 && l.fx >= 1 && l.fx <= 10 && (l.ch == 128 || l.ch == 64 || l.ch == 32 || l.ch == 16));
        EXPECT(l.lds_bytes == n * l.fy * l.fx * (l.ch + 4) * 4 && l.lds_bytes <= MBN_RESAMPLE_ENSEMBLE_LDS);
        EXPECT(l.tiles == 12 * 16 && l.span == 375 * 500);
        free(v);
    }
    /* the largest staging: eight views at ratio 4 on a 10 x 14 map */
    mbn_view big[MBN_ENSEMBLE_MAX_VIEWS];
    memset(big, 0, sizeof big);
    for (int k = 0; k < MBN_ENSEMBLE_MAX_VIEWS; k++) { big[k].x = 64 * (k % 4); big[k].y = 160 * (k / 4); big[k].iw = 224; big[k].ih = 160; big[k].mirror = k & 1; }
    EXPECT(mbn_resample_ensemble_envelope(2, 10, 14, 21, 320, 448, big, 8, 20, 28) == MBN_OK);
    mbn_resample_launch_t l;
    EXPECT(mbn_resample_ensemble_plan(10, 14, 320, 448, big, 8, 20, 28, &l) == MBN_OK);
    EXPECT(l.fy == 10 && l.fx == 10 && l.ch == 16 && l.lds_bytes == 64000);
    /* the refusals, the extreme arguments among them */
    mbn_view v;
    EXPECT(mbn_fit_view(45, 60, 64, 96, 0.0f, 0, &v) == MBN_EINVAL && mbn_fit_view(45, 60, 64, 96, 1.5f, 0, &v) == MBN_EINVAL);
    EXPECT(mbn_fit_view(45, 60, 64, 96, NAN, 0, &v) == MBN_EINVAL && mbn_fit_view(45, 60, 64, 96, 1.0f, 2, &v) == MBN_EINVAL);
    EXPECT(mbn_fit_view(45, 60, 64, 96, 1.0f, 0, NULL) == MBN_EINVAL && mbn_fit_view(0, 60, 64, 96, 1.0f, 0, &v) == MBN_EINVAL);
    EXPECT(mbn_fit_view(45, 60, 64, 96, 0.001f, 0, &v) == MBN_EINVAL);
    EXPECT(mbn_fit_view(8192, 1, 32, 32, 1.0f, 0, &v) == MBN_EINVAL);                                 /* an empty inner side */
    EXPECT(mbn_fit_view(2147483647, 1, 2147483647, 2147483647, 1.0f, 0, &v) == MBN_OK && v.iw == 1 && v.x == 1073741823);
    EXPECT(mbn_fit_view(2147483647, 2147483647, 2147483647, 2147483647, 1.0f, 1, &v) == MBN_OK && v.iw == 2147483647);
    EXPECT(mbn_resample_ensemble_envelope(2, 10, 14, 21, 320, 448, big, 0, 20, 28) == MBN_EINVAL);
    EXPECT(mbn_resample_ensemble_envelope(2, 10, 14, 21, 320, 448, big, 9, 20, 28) == MBN_EINVAL);
    EXPECT(mbn_resample_ensemble_envelope(2, 10, 14, 21, 320, 448, NULL, 1, 20, 28) == MBN_EINVAL);
    EXPECT(mbn_resample_ensemble_envelope(2147483647, 10, 14, 21, 320, 448, big, 8, 20, 28) == MBN_EUNSUPPORTED);
    EXPECT(mbn_resample_ensemble_envelope(2, 10, 14, 21, 320, 448, big, 8, 19, 28) == MBN_EUNSUPPORTED);
    big[7].x = 2147483647;                                                                            /* x + iw past int32 */
    EXPECT(mbn_resample_ensemble_envelope(2, 10, 14, 21, 320, 448, big, 8, 20, 28) == MBN_EINVAL);
    big[7].x = 0; big[7].reserved[2] = 1;
    EXPECT(mbn_resample_ensemble_envelope(2, 10, 14, 21, 320, 448, big, 8, 20, 28) == MBN_EINVAL);
    EXPECT(mbn_resample_ensemble_plan(10, 14, 320, 448, big, 0, 20, 28, &l) == MBN_EINVAL);
    EXPECT(mbn_resample_ensemble_plan(10, 14, 320, 448, big, 8, 20, 28, NULL) == MBN_EINVAL);
    EXPECT(mbn_resample_ensemble_plan(10, 14, 320, 448, NULL, 8, 20, 28, &l) == MBN_EINVAL);
    printf("ensemble host check: ok\n");
    return 0;
}
