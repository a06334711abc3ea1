/*
 * slide_host_check.c — the host side of the sliding-window read-out under the sanitizers: mbn_slide_axis, mbn_slide_plan,
 * mbn_resample_slide_envelope, mbn_slide_cells and mbn_resample_slide_plan, once each over the cases the tests name, from a program of its own
 * (no Python, no GPU):
 *
 *   PKG=cnn-mobilenet-v1-implementation-on-aws-fpga-using-opencl_amd
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$PKG/host tools/slide_host_check.c \
 *       $PKG/host/mbn_envelope.c $PKG/host/mbn_resize.c -lm -o /tmp/slide_host_check && /tmp/slide_host_check
 *
 * Exit status 0 and "slide host check: ok" when every answer is the expected one and the sanitizers saw nothing.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mbn.h"
#include "mbn_envelope.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

/* the two-line rule, written out again */
static int rule(int size, int tile, int stride, int *pos)
{
    const int n = (size > tile ? (size - tile + stride - 1) / stride : 0) + 1;
    for (int i = 0; i < n && i < MBN_SLIDE_MAX_AXIS; i++) pos[i] = i * stride < size - tile ? i * stride : size - tile;
    return n;
}

static mbn_slide hand(int th, int tw, int ny, const int *y, int nx, const int *x)
{
    mbn_slide s;
    memset(&s, 0, sizeof s);
    s.tile_rows = th; s.tile_cols = tw; s.ny = ny; s.nx = nx;
    for (int i = 0; i < ny && i < MBN_SLIDE_MAX_AXIS; i++) s.y[i] = y[i];
    for (int i = 0; i < nx && i < MBN_SLIDE_MAX_AXIS; i++) s.x[i] = x[i];
    return s;
}

int main(void)
{
    /* the sweep of the tests: positions on the heap, exactly as many as the rule gives: a write past the last one is the sanitizer's to find */
    long checked = 0;
    for (int tile = 4; tile <= 40; tile++)
        for (int stride = (tile + 1) / 2; stride <= tile; stride++)
            for (int size = tile; size <= 6 * tile + 6; size++) {
                int want[MBN_SLIDE_MAX_AXIS];
                const int n = rule(size, tile, stride, want);
                int32_t count = -1;
                if (n > MBN_SLIDE_MAX_AXIS) {
                    int32_t none[1] = { -7 };
                    EXPECT(mbn_slide_axis(size, tile, stride, none, &count) == MBN_EUNSUPPORTED && count == -1 && none[0] == -7);
                    continue;
                }
                int32_t *pos = malloc(sizeof(int32_t) * (size_t)n);
                EXPECT(pos != NULL);
                EXPECT(mbn_slide_axis(size, tile, stride, pos, &count) == MBN_OK && count == n);
                for (int i = 0; i < n; i++) EXPECT(pos[i] == want[i]);
                EXPECT(pos[0] == 0 && pos[n - 1] == size - tile);
                for (int i = 0; i + 1 < n; i++) EXPECT(pos[i + 1] > pos[i] && pos[i + 1] <= pos[i] + tile);
                for (int i = 0; i + 3 < n; i++) EXPECT(pos[i + 3] >= pos[i] + tile);                  /* three over a coordinate at most */
                /* the cells: tables on the heap of exactly MBN_SLIDE_MAX_CELLS + 1 entries */
                int32_t *edge = malloc(sizeof(int32_t) * (MBN_SLIDE_MAX_CELLS + 1)), *pieces = malloc(sizeof(int32_t) * (MBN_SLIDE_MAX_CELLS + 1)), kmax = 0;
                EXPECT(edge != NULL && pieces != NULL);
                const int cells = mbn_slide_cells(pos, n, tile, edge, pieces, &kmax);
                EXPECT(cells >= 1 && cells <= 2 * n - 1 && edge[0] == 0 && edge[cells] == size && kmax >= 1 && kmax <= 3 && pieces[0] == 0);
                for (int c = 0; c < cells; c++) EXPECT(edge[c + 1] > edge[c] && pieces[c + 1] == pieces[c] + (edge[c + 1] - edge[c] + 31) / 32);
                for (int c = cells + 1; c <= MBN_SLIDE_MAX_CELLS; c++) EXPECT(edge[c] == 0 && pieces[c] == 0);
                free(edge); free(pieces); free(pos);
                checked++;
            }
    EXPECT(checked > 50000);
    int32_t p3[3], n3 = 0;
    EXPECT(mbn_slide_axis(1000, 512, 341, p3, &n3) == MBN_OK && n3 == 3 && p3[0] == 0 && p3[1] == 341 && p3[2] == 488);
    /* the statuses of an axis, the extreme arguments among them; nothing is written on a refusal */
    int32_t pos[MBN_SLIDE_MAX_AXIS], n = -5;
    for (int i = 0; i < MBN_SLIDE_MAX_AXIS; i++) pos[i] = -5;
    EXPECT(mbn_slide_axis(0, 4, 4, pos, &n) == MBN_EINVAL && mbn_slide_axis(10, 0, 4, pos, &n) == MBN_EINVAL && mbn_slide_axis(10, 4, 0, pos, &n) == MBN_EINVAL);
    EXPECT(mbn_slide_axis(-1, 4, 4, pos, &n) == MBN_EINVAL && mbn_slide_axis(10, 4, 5, pos, &n) == MBN_EINVAL);
    EXPECT(mbn_slide_axis(10, 4, 4, NULL, &n) == MBN_EINVAL && mbn_slide_axis(10, 4, 4, pos, NULL) == MBN_EINVAL);
    EXPECT(mbn_slide_axis(10, 11, 11, pos, &n) == MBN_EUNSUPPORTED && mbn_slide_axis(100, 9, 4, pos, &n) == MBN_EUNSUPPORTED);
    EXPECT(mbn_slide_axis(69, 4, 4, pos, &n) == MBN_EUNSUPPORTED && mbn_slide_axis(2147483647, 1, 1, pos, &n) == MBN_EUNSUPPORTED);
    EXPECT(mbn_slide_axis(2147483647, 2147483647, 1073741824, pos, &n) == MBN_OK && n == 1 && pos[0] == 0);
    n = -5; pos[0] = -5;
    EXPECT(mbn_slide_axis(2147483647, 2147483646, 1073741823, pos, &n) == MBN_OK && n == 2 && pos[1] == 1);
    n = -5; pos[0] = pos[1] = -5;
    EXPECT(mbn_slide_axis(2147483647, 3, 2, pos, &n) == MBN_EUNSUPPORTED);
    for (int i = 0; i < MBN_SLIDE_MAX_AXIS; i++) EXPECT(pos[i] == -5);
    EXPECT(n == -5);
    /* the plan: filled whole, the unused entries 0; untouched on a refusal */
    mbn_slide *s = malloc(sizeof *s);
    EXPECT(s != NULL);
    memset(s, 0xAB, sizeof *s);
    EXPECT(mbn_slide_plan(85, 131, 40, 61, 20, 62, s) == MBN_EINVAL && mbn_slide_plan(85, 131, 90, 61, 20, 62, s) == MBN_EINVAL);
    EXPECT(mbn_slide_plan(85, 131, 90, 61, 45, 31, s) == MBN_EUNSUPPORTED && mbn_slide_plan(85, 131, 40, 61, 20, 30, s) == MBN_EUNSUPPORTED);
    for (size_t i = 0; i < sizeof *s; i++) EXPECT(((const unsigned char *)s)[i] == 0xAB);
    EXPECT(mbn_slide_plan(85, 131, 40, 61, 20, 31, NULL) == MBN_EINVAL);
    EXPECT(mbn_slide_plan(85, 131, 40, 61, 20, 31, s) == MBN_OK && s->ny == 4 && s->nx == 4 && s->y[3] == 45 && s->x[3] == 70 && s->tile_cols == 61);
    for (int i = 4; i < MBN_SLIDE_MAX_AXIS; i++) EXPECT(s->y[i] == 0 && s->x[i] == 0);
    /* the three geometry cases of the GPU test: envelope and launch */
    mbn_resample_launch_t l;
    memset(&l, 0xAB, sizeof l);
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 64, s, 85, 131) == MBN_OK && mbn_resample_slide_plan(2, 3, s, 85, 131, &l) == MBN_OK);
    EXPECT(l.fy == 2 && l.fx == 3 && l.ch == 128 && l.lds_bytes == 9 * 6 * 132 * 4 && l.tiles == 6 * 7 && l.span == 85 * 131);
    EXPECT(mbn_slide_plan(17, 25, 8, 12, 4, 6, s) == MBN_OK && mbn_resample_slide_envelope(2, 2, 3, 21, s, 17, 25) == MBN_OK);
    EXPECT(mbn_resample_slide_plan(2, 3, s, 17, 25, &l) == MBN_OK && l.tiles == 36 && l.lds_bytes <= MBN_RESAMPLE_ENSEMBLE_LDS);
    EXPECT(mbn_slide_plan(230, 333, 100, 150, 60, 90, s) == MBN_OK && mbn_resample_slide_envelope(2, 5, 7, 21, s, 230, 333) == MBN_OK);
    EXPECT(mbn_resample_slide_plan(5, 7, s, 230, 333, &l) == MBN_OK && l.fy == 4 && l.fx == 4 && l.ch == 64 && l.tiles == 130);
    EXPECT(mbn_resample_slide_plan(5, 7, NULL, 230, 333, &l) == MBN_EINVAL && mbn_resample_slide_plan(5, 7, s, 230, 333, NULL) == MBN_EINVAL);
    free(s);
    /* the worst case: the minimum ratio, nine tiles over a piece, a 10 x 10 footprint: 8 classes a chunk, 43 200 bytes */
    const int q[4] = { 0, 14, 28, 42 };
    mbn_slide worst = hand(40, 40, 4, q, 4, q);
    EXPECT(mbn_resample_slide_envelope(1, 10, 10, 21, &worst, 82, 82) == MBN_OK && mbn_resample_slide_plan(10, 10, &worst, 82, 82, &l) == MBN_OK);
    EXPECT(l.fy == 10 && l.fx == 10 && l.ch == 8 && l.lds_bytes == 43200);
    /* hand-made plans: gap, not flush, a non-zero unused entry, four tiles over a coordinate, tile < 4 x map */
    const int y3[3] = { 0, 4, 9 }, x3[3] = { 0, 6, 13 }, gap[2] = { 0, 9 }, y8[3] = { 0, 4, 8 }, four[5] = { 0, 2, 4, 6, 9 }, full[17] = { 0 };
    mbn_slide ok = hand(8, 12, 3, y3, 3, x3), bad;
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &ok, 17, 25) == MBN_OK && mbn_slide_check(&ok, 17, 25) == MBN_OK);
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, NULL, 17, 25) == MBN_EINVAL && mbn_slide_check(NULL, 17, 25) == MBN_EINVAL);
    EXPECT(mbn_resample_slide_envelope(0, 2, 3, 21, &ok, 17, 25) == MBN_EINVAL && mbn_resample_slide_envelope(2, 2, 3, 21, &ok, 17, 0) == MBN_EINVAL);
    bad = hand(8, 12, 2, gap, 3, x3);
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 25) == MBN_EINVAL);
    bad = hand(8, 12, 3, y8, 3, x3);
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 25) == MBN_EINVAL);
    bad = ok; bad.y[15] = 1;
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 25) == MBN_EINVAL);
    bad = ok; bad.ny = 0;
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 25) == MBN_EINVAL);
    bad = hand(8, 12, 17, full, 3, x3);                                                               /* ny past the arrays: refused before a read */
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 25) == MBN_EINVAL);
    bad = ok; bad.ny = 2147483647;
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 25) == MBN_EINVAL);
    bad = ok; bad.tile_rows = 2147483647;
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 25) == MBN_EINVAL);
    bad = hand(8, 12, 5, four, 3, x3);
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 25) == MBN_EUNSUPPORTED);
    bad = hand(8, 12, 5, four, 2, gap);
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 21) == MBN_EUNSUPPORTED);               /* x = { 0, 9 } of 12 is flush with 21 columns */
    EXPECT(mbn_resample_slide_envelope(2, 2, 3, 21, &bad, 17, 22) == MBN_EINVAL);                      /* an MBN_EINVAL of x before an MBN_EUNSUPPORTED of y */
    EXPECT(mbn_resample_slide_envelope(2, 3, 3, 21, &ok, 17, 25) == MBN_EUNSUPPORTED && mbn_resample_slide_envelope(2, 2, 4, 21, &ok, 17, 25) == MBN_EUNSUPPORTED);
    EXPECT(mbn_resample_slide_envelope(7281, 2, 3, 21, &ok, 17, 25) == MBN_OK && mbn_resample_slide_envelope(7282, 2, 3, 21, &ok, 17, 25) == MBN_EUNSUPPORTED);
    EXPECT(mbn_resample_slide_envelope(2147483647, 2, 3, 21, &ok, 17, 25) == MBN_EUNSUPPORTED);
    const int one[1] = { 0 }, two[2] = { 0, 1 };
    bad = hand(16384, 12, 2, two, 3, x3);
    EXPECT(mbn_resample_slide_envelope(1, 2, 3, 21, &bad, 16385, 25) == MBN_EUNSUPPORTED);
    bad = hand(16384, 16384, 1, one, 1, one);
    EXPECT(mbn_resample_slide_envelope(1, 2, 3, 21, &bad, 16384, 16384) == MBN_OK);
    EXPECT(mbn_resample_slide_plan(2, 3, &bad, 16384, 16384, &l) == MBN_OK && l.tiles == 512 * 512 && l.span == (int64_t)16384 * 16384);
    printf("slide host check: ok\n");
    return 0;
}
