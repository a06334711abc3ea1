/*
 * mbn_envelope.h — the shapes each fused kernel accepts, written down once. Pure predicates: no pointers, no context, no HIP;
 * each returns MBN_OK or MBN_EUNSUPPORTED. The C-ABI (csrc/mbn_abi.hip) asks them before it launches a fused kernel and the net
 * runner (host/mbn_net.c) when it plans, so the launches it lists are the ones that run. Pointer rules, the batch and tile
 * heuristics and the consistency between layers stay with the callers. Exported by libmbn.so and libmbn_host.so, not in mbn.h.
 */
#pragma once
#include <stdint.h>

#include "mbn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fused depthwise -> pointwise block (mbn_f32_dwpw*.hip, mbn_bf16_dwpw*.hip) */
#define MBN_CMAX 1024                /* largest Cin: the depthwise constants stay resident in LDS (44 KB) */
#define MBN_COUT_MAX 1024            /* largest Cout: its scale / shift stay resident in LDS */
#define MBN_OOB 0xF0000000u          /* byte offset beyond any supported tensor: a buffer load there returns zeros, so inputs stay below it */
/* full-rate window offsets (csrc/mbn_block_window.h): a tap's offset is (row term) + (column term), and a tap outside the image carries one of
 * these instead. Any sum with one of them lies in [MBN_OFF_BAD_COL, MBN_OOB + a little): beyond the descriptor's num_records and without
 * wrapping, as long as every input byte offset plus one left-pad column stays below MBN_OFF_BAD_COL: mbn_block_fast_offsets */
#define MBN_OFF_BAD_ROW 0x80000000u
#define MBN_OFF_BAD_COL 0x70000000u
/* bf16 resident run (mbn_bf16_res.hip): pixel rows of its two LDS images, the map with its border and the map, and blocks per launch */
#define MBN_RES_XPIX 144
#define MBN_RES_YROWS 104
#define MBN_RES_MAXBLK 8
#define MBN_TAIL_MAXSIDE 10          /* bf16 resident tail (mbn_bf16_tail.hip): largest side of its input map */
#define MBN_STEM_TH 8                /* fused stem (mbn_f32_stem.hip): output tile of a workgroup */
#define MBN_STEM_TW 16
/* dense head read-out (mbn_f32_dense.hip): a workgroup owns a 32 x 32 output tile of a grid that starts factor / 2 before the image; tiles along
 * an axis of n coarse samples, and the most tiles a launch can have (HIP: grid.x * 256 lanes below 2^32; the batch is grid.y, below 2^16) */
#define MBN_DENSE_TILE 32
#define MBN_DENSE_TILES(n, factor) (((n) * (factor) + (factor) / 2 + MBN_DENSE_TILE - 1) / MBN_DENSE_TILE)
#define MBN_DENSE_MAX_TILES 0xFFFFFFL
#define MBN_DENSE_MAX_BATCH 65535
/* dense head read-out at any output size (mbn_f32_resample.hip): a workgroup owns a 32 x 32 output tile (unshifted). The output is at least
 * MBN_RESAMPLE_MIN_RATIO times the coarse map on both axes and at most MBN_RESAMPLE_MAX_OUT a side ((2o + 1) * n then stays inside int32 and
 * den = 2N is exact). MBN_RESAMPLE_FOOT: the coarse samples a tile touches along an axis of n samples and N outputs at most: the source span of 32
 * outputs is 31 n / N, so i0 takes at most floor(31 n / N) + 2 values and i1 one more (10 at ratio 4, 6 at ratio 8). MBN_RESAMPLE_CH: the class
 * chunk of a launch whose tiles stage nv vectors: 128 while eight workgroups of nv * 132 floats fit a CU's 160 KB, else 64 (100 vectors: 27 KB, five
 * workgroups) */
#define MBN_RESAMPLE_TILE 32
#define MBN_RESAMPLE_MIN_RATIO 4
#define MBN_RESAMPLE_MAX_OUT 16384
#define MBN_RESAMPLE_FOOT(n, N) (31 * (n) / (N) + 3 < (n) ? 31 * (n) / (N) + 3 : (n))
#define MBN_RESAMPLE_CH(nv) ((nv) * 132 * 4 <= 20 * 1024 ? 128 : 64)

/* one 3x3 depthwise (stride, zero padding pad_top / pad_left) -> 1x1 pointwise block on `batch` NHWC images */
typedef struct mbn_block_shape {
    int batch, in_rows, in_cols, out_rows, out_cols, cin, cout, stride, pad_top, pad_left;
} mbn_block_shape;

/* mbn_dwpw_fused (dtype MBN_DT_F32) and mbn_dwpw_fused_bf16 (MBN_DT_BF16) */
int mbn_block_envelope(const mbn_block_shape *s, int dtype);
/* a block inside mbn_block_envelope whose window offsets may take the full-rate form (the unified-wave kernels' FO instantiations; one of the
 * terms of mbn_f32_dwpw3_eligible); the others run on the general form */
int mbn_block_fast_offsets(const mbn_block_shape *s, int dtype);
/* one block of a run of `nblocks` (mbn_blocks_resident_bf16): stride 1, pad 1, the map and the channels unchanged */
int mbn_resident_envelope(const mbn_block_shape *s, int nblocks);
/* the two blocks of mbn_tail_resident_bf16: b0 stride 2 without top / left padding on an even map, b1 stride 1 with pad 1 on b0's output */
int mbn_tail_envelope(const mbn_block_shape *b0, const mbn_block_shape *b1);
/* mbn_stem_fused_hw: c1 -> c1 -> c3 channels on rows x cols images; mbn_stem_envelope is the square form (mbn_stem_fused, _u8, _ex) */
int mbn_stem_envelope_hw(int batch, int rows, int cols, int c1, int c3);
int mbn_stem_envelope(int batch, int res, int c1, int c3);
/* mbn_upsample_argmax_f32: fp32 logits [batch][rows][cols][classes] -> labels (and scores) [batch][rows * factor][cols * factor]. factor 8, 16 or 32;
 * an image's logits and an image's output map each below 2^31 bytes (32-bit offsets inside an image; the batch goes through a 64-bit base) */
int mbn_upsample_argmax_envelope(int batch, int rows, int cols, int classes, int factor);
/* mbn_resample_argmax_f32: fp32 logits [batch][rows][cols][classes] -> labels (and scores) [batch][out_rows][out_cols]. MBN_EINVAL for a
 * non-positive size; else MBN_EUNSUPPORTED unless out_rows >= 4 rows, out_cols >= 4 cols, both at most 16384, an image's logits and an image's
 * output map each below 2^31 bytes, its tiles below 2^24 and batch at most 65535 */
int mbn_resample_argmax_envelope(int batch, int rows, int cols, int classes, int out_rows, int out_cols);
/* mbn_resample_softmax_f32 / _window_f32 / _ragged_f32: their shape checks are the argmax calls' above and below; this is the rest. MBN_EINVAL
 * unless min_prob is in [0, 1] (a NaN is not) and, without a prob map (have_prob == 0), min_prob > 0: without either the call is the argmax one */
int mbn_softmax_readout_check(int have_prob, float min_prob);
/* what a launch of that kernel needs. mbn_resample_plan WIDENS *l by one output size of a rows x cols map (zero it first): fy, fx = the LDS
 * footprint in vectors, ch = the class chunk, lds_bytes = fy * fx * (ch + 4) * 4, tiles = grid.x, span = elements of labels / score reached */
typedef struct mbn_resample_launch_t {
    int32_t fy, fx, ch, lds_bytes, tiles;
    int64_t span;
} mbn_resample_launch_t;
void mbn_resample_plan(int rows, int cols, int out_rows, int out_cols, mbn_resample_launch_t *l);
/* the items of one ragged set (mbn_ragged_readout_set) over a rows x cols x classes map: MBN_EINVAL for a non-positive size, a negative
 * dst_offset or two items whose maps overlap; MBN_EUNSUPPORTED for an item outside the per-image part of mbn_resample_argmax_envelope or a batch
 * above 65535. sort: scratch of 2 * batch int64. *l: the launch of the whole batch (span = max(dst_offset + rows * cols)) */
int mbn_resample_ragged_check(int rows, int cols, int classes, const mbn_label_item *items, int batch, int64_t *sort, mbn_resample_launch_t *l);
/* mbn_resample_argmax_window_f32: the same read-out of the window rect = (x, y, iw, ih) of the in_rows x in_cols network input that the rows x cols
 * map covers. MBN_EINVAL: a non-positive size, a NULL rect, x < 0, y < 0, iw < 1, ih < 1, x + iw > in_cols, y + ih > in_rows, in_rows < rows or
 * in_cols < cols. Else MBN_EUNSUPPORTED unless out_rows * in_rows >= 4 * ih * rows and out_cols * in_cols >= 4 * iw * cols, the output sides,
 * in_rows and in_cols are at most MBN_RESAMPLE_MAX_OUT (num < 2^46 and den <= 2^29 of the window rule are then exact in fp64) and the byte, tile
 * and batch limits of mbn_resample_argmax_envelope hold. MBN_RESAMPLE_WINDOW_FOOT: MBN_RESAMPLE_FOOT with n / N replaced by l n / (N R), in
 * 64-bit: the coarse samples 32 aligned outputs touch along an axis; for the full window (l = R) it is MBN_RESAMPLE_FOOT(n, N). */
#define MBN_RESAMPLE_WINDOW_FOOT(n, N, R, l) \
    (31 * (int64_t)(l) * (n) / ((int64_t)(N) * (R)) + 3 < (n) ? (int)(31 * (int64_t)(l) * (n) / ((int64_t)(N) * (R))) + 3 : (n))
int mbn_resample_window_envelope(int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows,
                                 int out_cols);
/* mbn_resample_plan for a window: widens *l likewise, with the window's footprint. The full window gives exactly mbn_resample_plan's answer */
void mbn_resample_window_plan(int rows, int cols, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols,
                              mbn_resample_launch_t *l);
/* mbn_resample_ragged_check for the items of mbn_ragged_readout_set_window: the same statuses, overlap sort and scratch, every item under
 * mbn_resample_window_envelope with its own rectangle; *l is written only when the batch is accepted */
int mbn_resample_ragged_window_check(int rows, int cols, int classes, int in_rows, int in_cols, const mbn_label_window_item *items, int batch,
                                     int64_t *sort, mbn_resample_launch_t *l);
/* mbn_resample_ensemble_f32: the read-out of n_views views of `batch` images (logits [n_views][batch][rows][cols][classes]). MBN_EINVAL: a
 * non-positive size, NULL views, n_views outside 1..MBN_ENSEMBLE_MAX_VIEWS, a view whose mirror is not 0 / 1, whose reserved words are not 0 or
 * whose rectangle mbn_resample_window_envelope calls MBN_EINVAL. Else MBN_EUNSUPPORTED when any view is outside mbn_resample_window_envelope taken
 * with batch * n_views images: one bad view refuses the set (an MBN_EINVAL of any view goes before an MBN_EUNSUPPORTED of another).
 * The plan WIDENS nothing: it writes *l for the whole set. fy, fx = the largest footprint over the views; the kernel stages all n_views footprints
 * per class chunk, view k at k * fy * fx vectors, so ch = MBN_RESAMPLE_ENSEMBLE_CH(n_views * fy * fx): the largest of 128 / 64 / 32 / 16 whose
 * staged block nv * (ch + 4) * 4 bytes stays at or under 64 KB, what a launch gets without asking for more and what leaves two workgroups on a CU.
 * Every set inside the envelope fits: 8 views x 10 x 10 vectors x 20 floats = 64 000 bytes. lds_bytes = n_views * fy * fx * (ch + 4) * 4; tiles
 * and span are those of one out_rows x out_cols map. MBN_EINVAL for NULL views / l or n_views outside 1..8 */
#define MBN_RESAMPLE_ENSEMBLE_LDS 65536
#define MBN_RESAMPLE_ENSEMBLE_CH(nv) \
    ((nv) * 132 * 4 <= MBN_RESAMPLE_ENSEMBLE_LDS ? 128 : (nv) * 68 * 4 <= MBN_RESAMPLE_ENSEMBLE_LDS ? 64 : (nv) * 36 * 4 <= MBN_RESAMPLE_ENSEMBLE_LDS ? 32 : 16)
int mbn_resample_ensemble_envelope(int batch, int rows, int cols, int classes, int in_rows, int in_cols, const mbn_view *views, int n_views,
                                   int out_rows, int out_cols);
int mbn_resample_ensemble_plan(int rows, int cols, int in_rows, int in_cols, const mbn_view *views, int n_views, int out_rows, int out_cols,
                               mbn_resample_launch_t *l);
/* mbn_resample_slide_f32: the read-out of a grid of tiles (include/mbn.h, "segment by sliding window"; logits [batch][ny * nx][rows][cols][classes]).
 * The envelope: MBN_EINVAL for a non-positive size, a NULL plan or a plan breaking the MBN_EINVAL rules of include/mbn.h for out_rows x out_cols
 * (either axis); else MBN_EUNSUPPORTED for more than three tiles over a coordinate, an output side above MBN_RESAMPLE_MAX_OUT, an output map of
 * 2^31 bytes or more, or a tile outside mbn_resample_argmax_envelope taken with batch * ny * nx maps resampled to tile_rows x tile_cols (the
 * ratio, the logits' bytes, the batch).
 * mbn_slide_cells: the tile edges cut an axis into cells of constant coverage, at most MBN_SLIDE_MAX_CELLS. edge[0 .. cells] are the cells'
 * borders (edge[0] = 0, edge[cells] = the axis' size), pieces[c] the 32-output pieces in front of cell c (pieces[cells]: of the axis), *kmax the
 * most tiles over a coordinate; the entries past `cells` are 0. Returns the number of cells; the axis is one the envelope accepts.
 * The plan writes *l for the whole grid: fy, fx = MBN_RESAMPLE_FOOT of a tile, which holds for ANY 32 consecutive outputs, so also for a piece
 * that starts at a cell border; the kernel stages the footprints of all tiles over a piece per class chunk, tile (ky, kx) of the piece at
 * (ky * Kx + kx) * fy * fx vectors, so ch = MBN_RESAMPLE_SLIDE_CH(K * fy * fx) with K = kmax_y * kmax_x of the plan: the largest of
 * 128 / 64 / 32 / 16 / 8 whose staged block stays at or under 64 KB (every plan inside the envelope fits: 9 x 10 x 10 vectors x 12 floats =
 * 43 200 bytes). lds_bytes = K * fy * fx * (ch + 4) * 4; tiles = pieces along y x pieces along x = grid.x; span = out_rows * out_cols.
 * MBN_EINVAL for a NULL plan / l; the plan is one the envelope accepts */
#define MBN_SLIDE_MAX_CELLS (2 * MBN_SLIDE_MAX_AXIS - 1)
#define MBN_RESAMPLE_SLIDE_CH(nv)                                                                                                  \
    ((nv) * 132 * 4 <= MBN_RESAMPLE_ENSEMBLE_LDS ? 128 : (nv) * 68 * 4 <= MBN_RESAMPLE_ENSEMBLE_LDS ? 64 : (nv) * 36 * 4 <= MBN_RESAMPLE_ENSEMBLE_LDS ? 32 \
     : (nv) * 20 * 4 <= MBN_RESAMPLE_ENSEMBLE_LDS ? 16 : 8)
int mbn_slide_check(const mbn_slide *s, int out_rows, int out_cols);      /* the plan's rules alone, for out_rows x out_cols */
int mbn_resample_slide_envelope(int batch, int rows, int cols, int classes, const mbn_slide *s, int out_rows, int out_cols);
int mbn_slide_cells(const int32_t *pos, int n, int tile, int32_t edge[MBN_SLIDE_MAX_CELLS + 1], int32_t pieces[MBN_SLIDE_MAX_CELLS + 1], int32_t *kmax);
int mbn_resample_slide_plan(int rows, int cols, const mbn_slide *s, int out_rows, int out_cols, mbn_resample_launch_t *l);
/* mbn_resample_topk_f32 (declared in mbn.h too): MBN_EINVAL for k outside 1..MBN_TOPK_MAX, k > classes and whatever the envelope of the same form
 * calls MBN_EINVAL (rect given: mbn_resample_window_envelope, NULL: mbn_resample_argmax_envelope; in_rows and in_cols are not read then); else that
 * envelope's MBN_EUNSUPPORTED; else MBN_EUNSUPPORTED when the k planes hold more than MBN_TOPK_MAX_ELEMENTS elements. The kernel reaches rank j of
 * image i through a 64-bit element base j * plane + i * map and 32-bit offsets inside a map, so nothing narrower than the base limits the planes;
 * 2^40 elements (4 TB an output, beyond any device) keeps k * plane inside int64 with room and every byte count of the span checks exact in a double.
 * mbn_resample_topk_ragged_check: the ragged form's part, for a set that reaches `span` elements: MBN_EINVAL for plane_stride < span, k as above;
 * MBN_EUNSUPPORTED for k * plane_stride above the same limit. The launch is the set's own (mbn_resample_window_plan / the handle's) */
#define MBN_TOPK_MAX_ELEMENTS ((int64_t)1 << 40)
int mbn_resample_topk_ragged_check(int classes, int64_t span, int k, int64_t plane_stride);
/* mbn_resample_nll_f32 (its envelope is declared in mbn.h too): MBN_EINVAL for truth_bytes other than 1 / 4, temps outside 1..MBN_NLL_MAX_TEMPS and
 * whatever the envelope of the same form calls MBN_EINVAL (rect given: mbn_resample_window_envelope, NULL: mbn_resample_argmax_envelope); else that
 * envelope's MBN_EUNSUPPORTED; else MBN_EUNSUPPORTED for classes > MBN_CONFUSION_MAX_CLASSES or temps planes above MBN_TOPK_MAX_ELEMENTS elements.
 * mbn_resample_nll_ragged_check: the ragged form's part, for a set that reaches `span` elements: MBN_EINVAL for plane_stride < span, then as above.
 * mbn_nll_temps_check: MBN_EINVAL for a NULL array, temps out of range or a beta that is NaN, infinite or outside [1/16, 16] */
int mbn_resample_nll_ragged_check(int classes, int64_t span, int truth_bytes, int temps, int64_t plane_stride);
int mbn_nll_temps_check(const float *inv_temps, int temps);
/* rank score (mbn_i32_topk_rank.hip, host/mbn_score.c; mbn_topk_metrics is declared in mbn.h). mbn_topk_rank_envelope: MBN_EINVAL for k outside
 * 1..MBN_TOPK_MAX, plane_stride < count or whatever mbn_confusion_envelope calls MBN_EINVAL, else its MBN_EUNSUPPORTED, and MBN_EUNSUPPORTED for
 * k * plane_stride above MBN_TOPK_MAX_ELEMENTS. mbn_topk_rank_form: MBN_CONFUSION_FORM_LDS while a workgroup's table of (classes + 1) * (k + 1)
 * 32-bit bins fits MBN_TOPK_RANK_LDS bytes (every class count of the envelope at every k: 4097 * 9 * 4 = 147 492 bytes would not, so the table
 * is capped at 48 KB, which leaves three workgroups of 1024 lanes a CU's LDS: up to 1364 classes at k = 8), MBN_CONFUSION_FORM_GLOBAL above */
#define MBN_TOPK_RANK_LDS (48 * 1024)
int mbn_topk_rank_envelope(int classes, int truth_bytes, int64_t count, int k, int64_t plane_stride);
int mbn_topk_rank_form(int classes, int k);
/* calibration score (mbn_f32_calibration.hip, host/mbn_score.c; declared in mbn.h too). mbn_calibration_envelope: MBN_EINVAL for bins < 1 or
 * whatever mbn_confusion_envelope calls MBN_EINVAL, else its MBN_EUNSUPPORTED, and MBN_EUNSUPPORTED for bins > MBN_CALIBRATION_MAX_BINS. One form:
 * a workgroup's table of (bins + 1) * 4 64-bit cells is at most 32 800 bytes of LDS */
int mbn_calibration_envelope(int classes, int truth_bytes, int bins, int64_t count);
/* score a segmentation (mbn_i32_confusion.hip, host/mbn_score.c; declared in mbn.h too). mbn_confusion_envelope: MBN_EINVAL for classes < 1,
 * count < 1 or truth_bytes other than 1 / 4, else MBN_EUNSUPPORTED for classes > MBN_CONFUSION_MAX_CLASSES or count > MBN_CONFUSION_MAX_COUNT.
 * mbn_confusion_form: MBN_CONFUSION_FORM_LDS while the workgroup's table of (classes + 1)^2 32-bit bins fits MBN_CONFUSION_LDS bytes of LDS,
 * that is up to MBN_CONFUSION_LDS_CLASSES (151^2 * 4 = 91 204 bytes: one workgroup of 16 waves on a CU; a table of at most half a CU's 160 KB, up to
 * 142 classes, leaves room for two), MBN_CONFUSION_FORM_GLOBAL above. MBN_CONFUSION_EPOCH: the chunks of 4096 pixels a workgroup counts between two flushes of
 * that table, so that a 32-bit bin stays below 2^32 */
#define MBN_CONFUSION_MAX_COUNT ((int64_t)1 << 34)
#define MBN_CONFUSION_LDS (92 * 1024)
#define MBN_CONFUSION_CU_LDS (160 * 1024)
#define MBN_CONFUSION_LDS_CLASSES 150
#define MBN_CONFUSION_EPOCH 512
#define MBN_CONFUSION_FORM_LDS 0
#define MBN_CONFUSION_FORM_GLOBAL 1
int mbn_confusion_envelope(int classes, int truth_bytes, int64_t count);
int mbn_confusion_form(int classes);
/* regions of a label map (mbn_i32_components.hip, host/mbn_regions.c; the functions are declared in mbn.h). MBN_COMPONENTS_TILE_ROWS x _COLS: the
 * tile a workgroup of the first kernel labels in LDS; MBN_COMPONENTS_CHUNK: the pixels of one unit of the flatten, numbering and write kernels, and
 * of one count of the two-level scan; MBN_COMPONENTS_MAX_PIXELS: what one handle may hold; an image stays below MBN_COMPONENTS_MAX_MAP pixels
 * (2^31 bytes of int32) */
#define MBN_COMPONENTS_TILE_ROWS 32
#define MBN_COMPONENTS_TILE_COLS 64
#define MBN_COMPONENTS_CHUNK 1024
#define MBN_COMPONENTS_MAX_PIXELS ((int64_t)1 << 34)
#define MBN_COMPONENTS_MAX_MAP ((int64_t)1 << 29)
/* panoptic quality (mbn_i32_panoptic.hip, host/mbn_panoptic.c; the functions are declared in mbn.h). MBN_PANOPTIC_CHUNK: the pixels of one unit of
 * the two pixel kernels (a wave holds 64 consecutive ones); MBN_PANOPTIC_BITS: the bits of a truth segment number (below
 * MBN_COMPONENTS_MAX_REGIONS = 2^24); MBN_PANOPTIC_SLOT_WORDS: the int32 words a predicted slot holds in the handle's scratch (non-void pixels, void
 * pixels, inter, one counter per bit), beside them one word for its candidate and one per truth slot; MBN_PANOPTIC_MAX_SLOTS: what one handle may
 * hold; MBN_PANOPTIC_LDS_CLASSES: up to that many classes a workgroup of the two deciding kernels counts its cells of pq_u64 in LDS (32 bytes a
 * class) and adds each to memory once, above it every segment adds to memory itself */
#define MBN_PANOPTIC_CHUNK 1024
#define MBN_PANOPTIC_BITS 24
#define MBN_PANOPTIC_SLOT_WORDS (3 + MBN_PANOPTIC_BITS)
#define MBN_PANOPTIC_LDS_CLASSES 1024
#define MBN_PANOPTIC_MAX_SLOTS ((int64_t)1 << 32)
/* boundary score (mbn_i32_boundary.hip, host/mbn_boundary.c; the functions are declared in mbn.h). Two half-width classes: d up to
 * MBN_BOUNDARY_SMALL_D takes tiles of MBN_BOUNDARY_SMALL_ROWS x MBN_BOUNDARY_TILE_COLS, a larger d tiles of MBN_BOUNDARY_LARGE_ROWS rows. A tile
 * keeps, per map, the value (4 bytes) and the horizontal distance (1 byte) of its own columns over its rows and d rows above and below:
 * (tile_rows + 2 d) * tile_cols * MBN_BOUNDARY_PIXEL_BYTES bytes of LDS, twice for the score kernel (truth and labels), which also holds
 * MBN_BOUNDARY_TABLE_BYTES of 32-bit bins: up to MBN_BOUNDARY_LDS_CLASSES classes a workgroup counts a tile there, (classes + 1)^2 trimap bins and
 * 3 * classes biou bins. MBN_BOUNDARY_MAX_MAP: a map stays below 2^29 pixels (indices are int32); MBN_BOUNDARY_MAX_BATCH: the maps of a uniform call */
#define MBN_BOUNDARY_SMALL_D 16
#define MBN_BOUNDARY_SMALL_ROWS 32
#define MBN_BOUNDARY_LARGE_ROWS 64
#define MBN_BOUNDARY_TILE_COLS 64
#define MBN_BOUNDARY_PIXEL_BYTES 5
#define MBN_BOUNDARY_LDS_CLASSES 31
#define MBN_BOUNDARY_TABLE_BYTES 4480
#define MBN_BOUNDARY_CU_LDS (160 * 1024)
#define MBN_BOUNDARY_MAX_MAP ((int64_t)1 << 29)
#define MBN_BOUNDARY_MAX_BATCH 65535
/* resize front-end (mbn_u8_resize.hip): one geometry of mbn_resizer_create. Source sides 1..8192, output sides 1..4096, at most MBN_RESIZE_MAX_KSIZE
 * taps per axis (a 32x downscale; any upscale has 3). box = (left, upper, right, lower), NULL = the whole image. MBN_EINVAL for a non-positive
 * size or a box mbn_resize_ksize refuses, else MBN_EUNSUPPORTED outside the limits. The batch (1..MBN_RESIZE_MAX_BATCH: grid.y) belongs to the call. */
#define MBN_RESIZE_MAX_IN 8192
#define MBN_RESIZE_MAX_OUT 4096
#define MBN_RESIZE_MAX_KSIZE 67
#define MBN_RESIZE_MAX_BATCH 65535
#define MBN_RESIZE_BITS 22           /* fractional bits of a weight: 32 - 8 - 2 */
#define MBN_RESIZE_HALF (1 << 21)    /* what a sum of weights x bytes starts from: it rounds to nearest */
int mbn_resize_envelope(int in_rows, int in_cols, const float *box, int out_rows, int out_cols);
/* The tile of both resize kernels (csrc/mbn_u8_resize.h is its body): a workgroup of MBN_RESIZE_WAVES waves owns toh x tow outputs of one image. tow
 * follows the output (MBN_RESIZE_TOW), toh is the tallest tile (MBN_RESIZE_TOH at most) whose LDS image fits MBN_RESIZE_LDS bytes: the tile's int32
 * tables, then at stage_off MBN_RESIZE_WAVES staged source rows of seg_stride bytes each, then at tmp_off the window [source rows][tow * 3] uint8.
 * The tables are, in this order,
 *   table kernel (mbn_u8_resize.hip)           wx [tow][kx], copied from the handle's tables; the other tables stay in memory
 *   ragged kernel (mbn_u8_resize_ragged.hip)   wx [tow][kx], wy [toh][ky], fx [tow], fy [toh], cy [toh], formed by the kernel: MBN_RESIZE_STAGE_OFF bytes
 * host/mbn_resize.c plans both from the exact lo / hi of every tile's two edge outputs (host/mbn_resize_axis.h), without a tap table. */
#define MBN_RESIZE_WAVES 4
#define MBN_RESIZE_TOH 32
#define MBN_RESIZE_LDS (60 * 1024)
#define MBN_RESIZE_TOW(out_cols) ((out_cols) <= 32 ? 32 : 64)
#define MBN_RESIZE_STAGE_OFF(tow, kx, toh, ky) ((4 * ((tow) * (kx) + (toh) * (ky) + (tow) + 2 * (toh)) + 15) & ~15)
typedef struct mbn_resize_plan_t {
    int32_t kx, ky;                  /* mbn_resize_ksize of the two axes */
    int32_t tow, toh;                /* columns and rows of a tile */
    int32_t tiles_x, tiles_y;        /* ceil(out_cols / tow), ceil(out_rows / toh) */
    int32_t seg_stride;              /* bytes of a staged row: the widest tile's segment + kx pixels of slack + 3, a multiple of 4 */
    int32_t stage_off, tmp_off;      /* LDS byte offsets of the staged rows and of the window */
    int32_t lds_bytes;               /* tmp_off + the tallest window * tow * 3 */
} mbn_resize_plan_t;
/* the table kernel's tile for one geometry (mbn_resizer_create): whatever mbn_resize_envelope answers, and MBN_EUNSUPPORTED when a tile of one
 * output row does not fit (no geometry inside the envelope does that) */
int mbn_resize_table_plan(int in_rows, int in_cols, const float *box, int out_rows, int out_cols, mbn_resize_plan_t *plan);
/* ragged resize (mbn_u8_resize_ragged.hip): every image of a launch has its own rows, cols and box, and its own plan in its descriptor. */
/* the descriptor of one image in device memory, 64 bytes: the caller's mbn_resize_item, then the plan */
typedef struct mbn_resize_desc {
    int64_t src_offset;              /* bytes from the launch's src pointer to the image's first byte */
    int32_t rows, cols;
    float box[4];                    /* left, upper, right, lower */
    int32_t kx, ky;                  /* mbn_resize_ksize of the two axes */
    int32_t toh, tiles_y;            /* rows of a tile; ceil(out_rows / toh) */
    int32_t wg0;                     /* the image's first workgroup: the prefix sum of tiles_x * tiles_y over the images before it */
    int32_t seg_stride;              /* bytes of a staged row: the widest tile's segment + kx pixels of slack + 3, a multiple of 4 */
    int32_t tmp_off;                 /* LDS byte offset of the window */
    int32_t lds_bytes;               /* tmp_off + the tallest window * tow * 3: what this image needs; a launch takes the largest of its batch */
} mbn_resize_desc;
/* [lo, hi): the source positions the outputs o_first..o_last of an axis reach, from the exact expressions of mbn_resize_taps at those two outputs only
 * (first[o_first] and first[o_last] + count[o_last] of the tables). MBN_EINVAL for what mbn_resize_ksize refuses or indices outside the axis */
int mbn_resize_window(int in_size, float b0, float b1, int out_size, int o_first, int o_last, int32_t *lo, int32_t *hi);
/* one image: MBN_EINVAL for a negative offset and whatever mbn_resize_envelope answers; fills *d (wg0 = 0). O(tiles) evaluations of lo / hi */
int mbn_resize_ragged_plan(const mbn_resize_item *item, int out_rows, int out_cols, mbn_resize_desc *d);
/* a batch: desc[i] with its wg0, the launch's workgroups (below 2^31, else MBN_EUNSUPPORTED) and dynamic LDS, and the bytes of src the batch reaches,
 * max(src_offset + rows * cols * 3). The first refused item's status is returned */
int mbn_resize_ragged_plan_batch(const mbn_resize_item *items, int batch, int out_rows, int out_cols, mbn_resize_desc *desc, int32_t *total_wgs,
                                 int32_t *lds_bytes, int64_t *src_span);
/* The same under a filter (MBN_FILTER_*, include/mbn.h; any other value: MBN_EINVAL): every function above is the MBN_FILTER_BILINEAR call of its
 * sibling here. The limits do not change with the filter; what changes is how soon they bind: support = S * fs widens the windows (S = 0.5 box,
 * 2 bicubic, 3 lanczos), so ksize <= 67 ends lanczos at 11x and bicubic at 16.5x, and box, whose 67 taps span 66 source positions, is ended by the
 * one-row tile that must fit MBN_RESIZE_LDS (the plan's MBN_EUNSUPPORTED). MBN_FILTER_NEAREST is a gather: ksize 1, a window is [index[o_first],
 * index[o_last] + 1), a table plan needs no LDS (kx = ky = 1, toh = min(out_rows, MBN_RESIZE_TOH), the offsets 0) and a ragged plan the tile's
 * tow + toh int32 indices. The ragged plans answer MBN_EUNSUPPORTED for MBN_FILTER_HAMMING and MBN_FILTER_LANCZOS (no device form of sin / cos
 * gives the host's bits) */
int mbn_resize_envelope_filter(int filter, int in_rows, int in_cols, const float *box, int out_rows, int out_cols);
int mbn_resize_table_plan_filter(int filter, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, mbn_resize_plan_t *plan);
int mbn_resize_window_filter(int filter, int in_size, float b0, float b1, int out_size, int o_first, int o_last, int32_t *lo, int32_t *hi);
int mbn_resize_ragged_plan_filter(int filter, const mbn_resize_item *item, int out_rows, int out_cols, mbn_resize_desc *d);
int mbn_resize_ragged_plan_batch_filter(int filter, const mbn_resize_item *items, int batch, int out_rows, int out_cols, mbn_resize_desc *desc,
                                        int32_t *total_wgs, int32_t *lds_bytes, int64_t *src_span);
/* The letterbox (mbn_fit_pad, include/mbn.h): the whole image resized to ih x iw into the rectangle (x, y, iw, ih) of an out_rows x out_cols canvas,
 * `fill` elsewhere. The tiles are those of the plain resize (H, W) -> (ih, iw), laid over the rectangle; the border is written by workgroups of its own,
 * each MBN_RESIZE_FILL_ROWS border rows of one canvas, a wave a row at a time. Border row k (of fill_rows) is canvas row k where the rectangle is
 * narrower than the canvas (every row has a border then) and otherwise the k-th row outside it: k above the rectangle, k + ih below it
 * (MBN_RESIZE_FILL_ROW). fill_wgs = ceil(fill_rows / MBN_RESIZE_FILL_ROWS): none where the aspect ratios agree. */
#define MBN_RESIZE_FILL_ROWS 32
#define MBN_RESIZE_FILL_ROW(k, y, iw, ih, ow) ((iw) < (ow) || (k) < (y) ? (k) : (k) + (ih))
/* the table form (mbn_resizer_create_pad): mbn_resize_table_plan_filter of (H, W) -> (ih, iw), the whole image, and the rectangle. Whatever
 * mbn_fit_pad and that plan answer */
typedef struct mbn_resize_pad_plan_t {
    mbn_resize_plan_t plan;          /* of the inner image: tow = MBN_RESIZE_TOW(iw), tiles_x * tiles_y tiles per image */
    int32_t x, y, iw, ih;            /* mbn_fit_pad */
    int32_t fill_rows, fill_wgs;     /* border rows of a canvas and the workgroups that write them: grid.x is tiles_x * tiles_y + fill_wgs */
} mbn_resize_pad_plan_t;
int mbn_resize_pad_table_plan_filter(int filter, int in_rows, int in_cols, int out_rows, int out_cols, mbn_resize_pad_plan_t *plan);
/* the same with the rectangle given (mbn_resizer_create_view): MBN_EINVAL for a NULL view, a rectangle outside the canvas, an empty side, a non-zero
 * reserved word or mirror outside 0 / 1, else that plan's answer for (H, W) -> (ih, iw). The mirror changes no tile and no border */
int mbn_resize_view_table_plan_filter(int filter, int in_rows, int in_cols, int out_rows, int out_cols, const mbn_view *view,
                                      mbn_resize_pad_plan_t *plan);
/* the ragged form (mbn_ragged_resizer_create_pad): the descriptor of one image in device memory, 96 bytes. img is mbn_resize_ragged_plan_filter of the
 * item against ih x iw, field for field (kx .. lds_bytes as for a plain ragged launch whose output is ih x iw); its wg0 is the image's first workgroup
 * of the pad launch, which gives the image tiles_x * tiles_y tile workgroups and then fill_wgs border workgroups. The inner size is the image's own, so
 * tow and tiles_x, which a plain launch has once per handle, are here too */
typedef struct mbn_resize_pad_desc {
    mbn_resize_desc img;
    int32_t x, y, iw, ih;            /* mbn_fit_pad of (rows, cols) into the handle's canvas */
    int32_t tow, tiles_x;            /* MBN_RESIZE_TOW(iw), ceil(iw / tow) */
    int32_t fill_rows, fill_wgs;     /* as in mbn_resize_pad_plan_t */
} mbn_resize_pad_desc;
/* one image (wg0 = 0): MBN_EINVAL for a negative offset, a box that is not the whole image or what mbn_fit_pad refuses, else what
 * mbn_resize_ragged_plan_filter answers for (rows, cols) -> (ih, iw) */
int mbn_resize_pad_ragged_plan_filter(int filter, const mbn_resize_item *item, int out_rows, int out_cols, mbn_resize_pad_desc *d);
/* a batch, as mbn_resize_ragged_plan_batch_filter: the launch's workgroups count every image's tiles and border workgroups */
int mbn_resize_pad_ragged_plan_batch_filter(int filter, const mbn_resize_item *items, int batch, int out_rows, int out_cols, mbn_resize_pad_desc *desc,
                                            int32_t *total_wgs, int32_t *lds_bytes, int64_t *src_span);

/* int8 pointwise / FC (mbn_i8.hip): the whole launch arithmetic of mbn_launch_i8_pointwise, which launches what this says and
 * computes nothing of its own. Two forms: the persistent one (i8_pw2_k<ks, 512, out_f32>: a wave keeps a 32-column chunk's filter
 * rows, the workgroup's gx * gy copies walk `ntiles` tiles of `pt` pixels grid-strided through two LDS buffers) and the
 * K-in-registers one (i8_pw_k<ks, g, out_f32>: a workgroup = 128 pixels x cpg chunks, K streamed in blocks of 32 * ks bytes). */
#define MBN_I8_PW_PERSISTENT 1
#define MBN_I8_PW_KREG 2
#define MBN_I8_PW_MAXWAVES 8         /* waves of a persistent workgroup at most */
#define MBN_I8_PW_LDS_MAX (160 * 1024)
typedef struct mbn_i8_pw_plan_t {
    int form;                        /* MBN_I8_PW_PERSISTENT or MBN_I8_PW_KREG */
    int ks;                          /* the kernel's KS: 32-byte k steps held in registers (1, 2, 4, 8, 16, 32; KREG: 4, 16, 32) */
    int g;                           /* bytes per global load of a row: 16 (K % 16 == 0) or 8; KREG: 16 only with the operands on 16 bytes */
    int out_f32;                     /* the OUTF32 instantiation */
    int pt;                          /* pixels per tile (PERSISTENT: a multiple of 32; KREG: 128) */
    int threads;                     /* per workgroup */
    int gy;                          /* grid.y: column groups of the PERSISTENT form (KREG: 1, its groups are folded into grid.x) */
    int lds_bytes;                   /* dynamic LDS (KREG: 0) */
    long ntiles;                     /* ceil(m / pt) */
    long gx;                         /* grid.x. PERSISTENT: workgroup x takes tiles x, x + gx, ...; KREG: ntiles * ngroups */
    /* PERSISTENT only (0 in a KREG plan) */
    int kp;                          /* K rounded up to 32: a row of a tile in LDS is kp + 16 bytes */
    int cpw, rep;                    /* waves = cpw chunks x rep groups of 32-pixel sub-tiles */
    int resident;                    /* workgroups a CU is counted to hold */
    int maxg;                        /* the kernel's MAXG: granules a thread stages per tile; pt * (K / g) <= maxg * threads */
    long per_round, rounds;          /* resident slots per column group; passes over them the largest tile needs */
    /* KREG only (0 in a PERSISTENT plan) */
    int nkb;                         /* K blocks of 32 * ks bytes */
    int nchunks, cpg, ngroups;       /* 32-column chunks, chunks per workgroup, workgroups per pixel tile */
} mbn_i8_pw_plan_t;
/* m pixels, K = cin (a multiple of 8), N = op_size on a device of num_cus CUs; operands_on_16: activations and filter on 16 bytes (they
 * are on 8 at least). MBN_EINVAL for a shape the C-ABI refuses before it, MBN_EUNSUPPORTED for a grid beyond 2^31 - 1 workgroups. */
int mbn_i8_pw_plan(long m, int cin, int op_size, int num_cus, int operands_on_16, int out_f32, mbn_i8_pw_plan_t *plan);

#ifdef __cplusplus
}
#endif
