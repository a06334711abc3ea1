/*
 * label_set_host_check.cpp — the unit walker of csrc/mbn_label_set.h under the sanitizers, on host copies of a ragged read-out set, from a
 * program of its own (no Python, no GPU):
 *
 *   PKG=cnn-mobilenet-v1-implementation-on-aws-fpga-using-opencl_amd
 *   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$PKG/host -I$PKG/csrc \
 *       tools/label_set_host_check.cpp -o /tmp/label_set_host_check && /tmp/label_set_host_check
 *
 * For sets of both item sizes (16 and 32 bytes) it walks every unit by tile, by chunk and by image and expects: the units of an image are
 * 0 .. per - 1, each once and in order; offsets and running sums equal a plain loop's; equal-sized items laid out one behind the other answer
 * as the uniform form does; the unit one past the end is "none". The blocks are heap memory of exactly head + items bytes, so a read past
 * the last item is the sanitizer's to report. Exit status 0 and "label set host check: ok".
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mbn_label_set.h"
#include "mbn_envelope.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

namespace {

constexpr int TR = MBN_COMPONENTS_TILE_ROWS, TC = MBN_COMPONENTS_TILE_COLS, CHUNK = MBN_COMPONENTS_CHUNK;

/* the rules of the kernel files */
inline long long tiles(int rows, int cols) { return (long long)((rows + TR - 1) / TR) * ((cols + TC - 1) / TC); }
inline long long chunks(int rows, int cols) { return ((long long)rows * cols + CHUNK - 1) / CHUNK; }

struct Map { int rows, cols; long long off; };

/* a block as the handle keeps it: head, then items of item_bytes each (the window fields of a 32-byte item are set to a pattern nothing reads) */
mbn_label_set make_set(const std::vector<Map> &maps, int item_bytes, int generation)
{
    const size_t bytes = sizeof(mbn_label_set_head) + maps.size() * (size_t)item_bytes;
    char *block = (char *)malloc(bytes);
    memset(block, 0x5a, bytes);
    mbn_label_set_head head = { (int32_t)maps.size(), generation, { 0, 0 } };
    memcpy(block, &head, sizeof head);
    for (size_t i = 0; i < maps.size(); i++) {
        const mbn_label_item it = { maps[i].off, maps[i].rows, maps[i].cols };
        memcpy(block + sizeof head + i * (size_t)item_bytes, &it, sizeof it);
    }
    return { (const mbn_label_set_head *)block, generation, item_bytes };
}

/* every unit of the call under PER, SUM = chunks, against a plain loop over the maps. uniform: the maps are `batch` equal ones, contiguous, and the
   uniform form must give the same answers */
template <mbn_label_units_fn PER>
int walk(const mbn_label_set &set, const std::vector<Map> &maps, bool uniform)
{
    const int batch = (int)maps.size(), rows = maps[0].rows, cols = maps[0].cols;
    long long u = 0, pixels = 0, sum = 0;
    for (int i = 0; i < batch; i++) {
        const long long per = PER(maps[i].rows, maps[i].cols);
        EXPECT(per >= 1);
        for (long long k = 0; k < per; k++, u++) {
            mbn_label_unit w;
            memset(&w, 0xff, sizeof w);
            EXPECT((mbn_label_set_unit<true, PER, chunks>(set, 0, 0, 0, u, w)));
            EXPECT(w.image == i && w.unit == k && w.rows == maps[i].rows && w.cols == maps[i].cols);
            EXPECT(w.off == maps[i].off && w.pixels == pixels && w.sum == sum);
            if (uniform) {
                mbn_label_unit v;
                memset(&v, 0xff, sizeof v);
                EXPECT((mbn_label_set_unit<false, PER, chunks>(set, batch, rows, cols, u, v)));
                EXPECT(v.image == w.image && v.unit == w.unit && v.rows == w.rows && v.cols == w.cols);
                EXPECT(v.off == w.off && v.pixels == w.pixels && v.sum == w.sum);
            }
        }
        pixels += (long long)maps[i].rows * maps[i].cols;
        sum += chunks(maps[i].rows, maps[i].cols);
    }
    /* one past the end, and far past it */
    mbn_label_unit w;
    EXPECT(!(mbn_label_set_unit<true, PER, chunks>(set, 0, 0, 0, u, w)) && !(mbn_label_set_unit<true, PER, chunks>(set, 0, 0, 0, u + (1ll << 40), w)));
    if (uniform) EXPECT(!(mbn_label_set_unit<false, PER, chunks>(set, batch, rows, cols, u, w)));
    return 0;
}

int check(const std::vector<Map> &maps, bool uniform)
{
    const int sizes[2] = { (int)sizeof(mbn_label_item), (int)sizeof(mbn_label_window_item) };
    for (int item_bytes : sizes) {
        const mbn_label_set set = make_set(maps, item_bytes, 7);
        EXPECT(!mbn_label_set_stale(set));
        mbn_label_set older = set;
        older.generation = 6;
        EXPECT(mbn_label_set_stale(older));
        for (size_t i = 0; i < maps.size(); i++) {
            const mbn_label_item *it = mbn_label_set_item(set, (int)i);
            EXPECT(it->rows == maps[i].rows && it->cols == maps[i].cols && it->dst_offset == maps[i].off);
        }
        int bad = walk<tiles>(set, maps, uniform);
        if (!bad) bad = walk<chunks>(set, maps, uniform);
        if (!bad) bad = walk<mbn_label_units_image>(set, maps, uniform);
        free((void *)set.head);
        if (bad) return bad;
    }
    return 0;
}

}   // namespace

int main(void)
{
    /* a ragged set: 1 x 1; exactly one chunk (one tile); exactly one tile (two chunks); one pixel, one row and one column more than those; an
       ordinary image. The offsets are not in order and leave gaps, as a caller's may */
    const int dims[][2] = { { 1, 1 }, { CHUNK / TC, TC }, { TR, TC }, { 25, 41 }, { CHUNK / TC + 1, TC }, { CHUNK / TC, TC + 1 }, { TR + 1, TC },
                            { TR, TC + 1 }, { 375, 500 }, { 1, CHUNK + 1 }, { CHUNK + 1, 1 } };
    EXPECT(25 * 41 == CHUNK + 1 && tiles(25, 41) == 1 && chunks(25, 41) == 2 && tiles(TR, TC) == 1 && chunks(CHUNK / TC, TC) == 1);
    std::vector<Map> ragged;
    long long off = 1000000;
    for (const auto &d : dims) {
        off -= (long long)d[0] * d[1] + 3;
        ragged.push_back({ d[0], d[1], off });
    }
    if (check(ragged, false)) return 1;
    /* equal maps one behind the other: the uniform form's answers. One image, and several, at each of the sizes above */
    for (const auto &d : dims)
        for (int batch : { 1, 3 }) {
            std::vector<Map> same;
            for (int i = 0; i < batch; i++) same.push_back({ d[0], d[1], (long long)i * d[0] * d[1] });
            if (check(same, true)) return 1;
        }
    printf("label set host check: ok\n");
    return 0;
}
