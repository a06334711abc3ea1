// mbn_label_set.h — the one view of a ragged read-out set: the block a mbn_ragged_readout handle keeps on the device and pinned on
// the host is a 16-byte head and behind it the items of the last set, mbn_label_item or mbn_label_window_item (the first 16 bytes of the latter
// are the former). mbn_f32_resample.hip writes the block; every consumer of a set (confusion, components, boundary, panoptic) reads it through
// what stands here: the head, the view a kernel's arguments carry, the item accessors, the walk from a unit of work to its image, and on the
// host the envelope walk over the items and the event behind a launch.
// The first part is plain C++ (a host program can walk a host copy of a set: tools/label_set_host_check.cpp); the second needs the handle.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mbn.h"

#ifdef __HIPCC__
#define MBN_SET_FN __host__ __device__ __forceinline__
#else
#define MBN_SET_FN inline
#endif

// head of the block, in front of the items
struct mbn_label_set_head {
    int32_t batch, generation, pad[2];
};
static_assert(sizeof(mbn_label_set_head) == 16 && sizeof(mbn_label_item) == 16 && sizeof(mbn_label_window_item) == 32 && sizeof(mbn_region) == 32,
              "device layout");
static_assert(offsetof(mbn_label_window_item, dst_offset) == offsetof(mbn_label_item, dst_offset) &&
              offsetof(mbn_label_window_item, rows) == offsetof(mbn_label_item, rows) &&
              offsetof(mbn_label_window_item, cols) == offsetof(mbn_label_item, cols), "a window item begins as a plain item");

// what a kernel's arguments carry of a set: the block, the generation the launch was made under and the bytes of one item
struct mbn_label_set {
    const mbn_label_set_head *head;
    int generation, item_bytes;
};

// item i of the block (plain loads: the items were uploaded before the launch)
MBN_SET_FN const mbn_label_item *mbn_label_set_item(const mbn_label_set &s, int i)
{
    return (const mbn_label_item *)((const char *)(s.head + 1) + (size_t)i * s.item_bytes);
}

// a launch captured under an earlier set and replayed after another: it has nothing to do
MBN_SET_FN bool mbn_label_set_stale(const mbn_label_set &s) { return s.head->generation != s.generation; }

// One unit of work of a kernel whose units are dealt over all images of a call: the image it lies in and its number inside that image
struct mbn_label_unit {
    long long off;        // the image's first element in the maps of the call
    long long pixels;     // the pixels of the images before it
    long long sum;        // SUM (rows, cols) over the images before it
    int rows, cols, image;
    int unit;
};

// a units-per-image rule: how many units an image of rows x cols has (tiles, chunks, ...); at least 1
typedef long long (*mbn_label_units_fn)(int rows, int cols);
MBN_SET_FN long long mbn_label_units_image(int, int) { return 1; }        // the image itself is the unit

// Unit u of a call whose images have PER units each; false when u is past the last one. Uniform form: `batch` images of rows x cols, one behind
// the other. Ragged form: the items of `set` (batch, rows and cols are not read). The uniform form is a division, the ragged form a walk over the
// items. SUM is a second rule, summed over the images in front (components: the chunks, whatever the unit is)
template <bool RAGGED, mbn_label_units_fn PER, mbn_label_units_fn SUM = PER>
MBN_SET_FN bool mbn_label_set_unit(const mbn_label_set &set, int batch, int rows, int cols, long long u, mbn_label_unit &w)
{
    if (!RAGGED) {
        const long long per = PER(rows, cols);
        const long long i = u / per;
        if (i >= batch) return false;
        w.image = (int)i;
        w.unit = (int)(u - i * per);
        w.rows = rows; w.cols = cols;
        w.off = w.pixels = i * ((long long)rows * cols);
        w.sum = i * SUM(rows, cols);
        return true;
    }
    const int n = set.head->batch;
    long long pixels = 0, sum = 0;
    for (int i = 0; i < n; i++) {
        const mbn_label_item *it = mbn_label_set_item(set, i);
        const int r = it->rows, c = it->cols;
        const long long per = PER(r, c);
        if (u < per) {
            w.image = i;
            w.unit = (int)u;
            w.rows = r; w.cols = c;
            w.off = it->dst_offset;
            w.pixels = pixels;
            w.sum = sum;
            return true;
        }
        u -= per;
        pixels += (long long)r * c;
        sum += SUM(r, c);
    }
    return false;
}

#ifdef __HIPCC__
#include "mbn_internal.h"

inline int mbn_ragged_readout_item_bytes(const mbn_ragged_readout *r)
{
    return r->window ? (int)sizeof(mbn_label_window_item) : (int)sizeof(mbn_label_item);
}

// the view of the handle's last set a launch passes to its kernel
inline mbn_label_set mbn_ragged_readout_view(const mbn_ragged_readout *r)
{
    return { (const mbn_label_set_head *)r->dev, r->generation, mbn_ragged_readout_item_bytes(r) };
}

// item i of the last set, as the handle's pinned block still holds it
inline const mbn_label_item *mbn_ragged_readout_item(const mbn_ragged_readout *r, int i)
{
    const mbn_label_set pinned = { (const mbn_label_set_head *)r->host, r->generation, mbn_ragged_readout_item_bytes(r) };
    return mbn_label_set_item(pinned, i);
}

// The answer of a ragged call's envelope over every item of the set: MBN_EINVAL wins, else the first refusal. check (item) -> MBN_*; it adds up
// what the call needs (tiles, chunks, pixels) of the items that pass
template <typename Check>
inline int mbn_ragged_readout_envelope(const mbn_ragged_readout *r, Check check)
{
    int shape = MBN_OK;
    for (int i = 0; i < r->batch; i++) {
        const int rc = check(*mbn_ragged_readout_item(r, i));
        if (rc == MBN_EINVAL || (rc != MBN_OK && shape == MBN_OK)) shape = rc;
    }
    return shape;
}

// Behind a launch that read the set: the next set waits for it. Inside a capture there is nothing to wait for (the replays are the caller's to order)
inline void mbn_ragged_readout_mark_done(mbn_ragged_readout *r, hipStream_t stream)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) (void)hipEventRecord(r->done, stream);
}
#endif
