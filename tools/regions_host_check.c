/*
 * regions_host_check.c — the host side of "regions of a label map" under the sanitizers: mbn_components_envelope, mbn_components_tile and
 * mbn_components_scratch_bytes over the cases the tests name, from a program of its own (no Python, no GPU):
 *
 *   PKG=cnn-mobilenet-v1-implementation-on-aws-fpga-using-opencl_amd
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$PKG/host tools/regions_host_check.c \
 *       $PKG/host/mbn_regions.c -o /tmp/regions_host_check && /tmp/regions_host_check
 *
 * Exit status 0 and "regions host check: ok" when every answer is the expected one and the sanitizers saw nothing.
 */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include "mbn.h"
#include "mbn_envelope.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main(void)
{
    /* the tile, into heap ints exactly as large as the call may touch */
    int *tr = malloc(sizeof(int)), *tc = malloc(sizeof(int));
    EXPECT(tr && tc);
    EXPECT(mbn_components_tile(tr, tc) == MBN_OK && *tr == MBN_COMPONENTS_TILE_ROWS && *tc == MBN_COMPONENTS_TILE_COLS);
    EXPECT(mbn_components_tile(NULL, tc) == MBN_EINVAL && mbn_components_tile(tr, NULL) == MBN_EINVAL);
    free(tr); free(tc);
    /* the envelope: every malformed argument, both limits from both sides, the products that would overflow an int */
    EXPECT(mbn_components_envelope(1, 1, 1, 1, 4, 1, 0) == MBN_OK && mbn_components_envelope(65535, 375, 500, 1000, 8, 50, 1 << 24) == MBN_OK);
    EXPECT(mbn_components_envelope(0, 4, 4, 2, 4, 1, 0) == MBN_EINVAL && mbn_components_envelope(1, 0, 4, 2, 4, 1, 0) == MBN_EINVAL);
    EXPECT(mbn_components_envelope(1, 4, -1, 2, 4, 1, 0) == MBN_EINVAL && mbn_components_envelope(1, 4, 4, 0, 4, 1, 0) == MBN_EINVAL);
    EXPECT(mbn_components_envelope(1, 4, 4, 2, 4, 0, 0) == MBN_EINVAL && mbn_components_envelope(1, 4, 4, 2, 4, 1, -1) == MBN_EINVAL);
    for (int conn = -9; conn <= 9; conn++)
        EXPECT(mbn_components_envelope(1, 4, 4, 2, conn, 1, 0) == (conn == 4 || conn == 8 ? MBN_OK : MBN_EINVAL));
    EXPECT(mbn_components_envelope(1, 1, (1 << 29) - 1, 2, 4, 1, 0) == MBN_OK && mbn_components_envelope(1, 1, 1 << 29, 2, 4, 1, 0) == MBN_EUNSUPPORTED);
    EXPECT(mbn_components_envelope(1, INT_MAX, INT_MAX, INT_MAX, 8, INT_MAX, 0) == MBN_EUNSUPPORTED);
    EXPECT(mbn_components_envelope(65536, 4, 4, 2, 4, 1, 0) == MBN_EUNSUPPORTED && mbn_components_envelope(INT_MAX, 4, 4, 2, 4, 1, 0) == MBN_EUNSUPPORTED);
    EXPECT(mbn_components_envelope(1, 4, 4, 2, 4, 1, (1 << 24) + 1) == MBN_EUNSUPPORTED && mbn_components_envelope(1, 4, 4, 2, 4, 1, INT_MAX) == MBN_EUNSUPPORTED);
    EXPECT(mbn_components_envelope(65536, 4, 4, 2, 6, 1, 0) == MBN_EINVAL);                                    /* a caller error goes before a limit */
    /* the scratch: 8 bytes a pixel and a small term, up to the largest handle; 0 for what create refuses */
    const int64_t big = MBN_COMPONENTS_MAX_PIXELS;
    EXPECT(mbn_components_scratch_bytes(1, 1) == 256 && mbn_components_scratch_bytes(65535, big) >= 8 * big);
    EXPECT(mbn_components_scratch_bytes(65535, big) <= 8 * big + big / 128 + 16 * 65535 + 256);
    EXPECT(mbn_components_scratch_bytes(32, 6000000) % 256 == 0 && mbn_components_scratch_bytes(32, 6000000) >= 48000000 + 4 * (5859 + 32));
    EXPECT(mbn_components_scratch_bytes(0, 10) == 0 && mbn_components_scratch_bytes(1, 0) == 0 && mbn_components_scratch_bytes(-1, -1) == 0);
    EXPECT(mbn_components_scratch_bytes(65536, 10) == 0 && mbn_components_scratch_bytes(1, big + 1) == 0 && mbn_components_scratch_bytes(INT_MAX, INT64_MAX) == 0);
    printf("regions host check: ok\n");
    return 0;
}
