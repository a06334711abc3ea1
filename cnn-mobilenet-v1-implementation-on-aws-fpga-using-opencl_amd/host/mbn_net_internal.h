/* mbn_net_internal.h — what the two halves of the net runner share: struct mbn_net and two functions. mbn_net.c is the runner (the launches of a
 * forward pass); mbn_net_segment.c is the segmentation family built on mbn_net_forward_dense, and owns the `seg` member. */
#ifndef MBN_NET_INTERNAL_H
#define MBN_NET_INTERNAL_H

#include "mbn.h"

/* what a source-size segment call wrote: the maps its consumers (mbn_net_segment_score, _regions, ...) work on */
enum { MBN_SEG_NONE = 0, MBN_SEG_UNIFORM = 1, MBN_SEG_RAGGED = 2 };
struct mbn_seg_maps {
    int kind;                       /* MBN_SEG_NONE until a call succeeds; _UNIFORM: [batch][rows][cols]; _RAGGED: the maps of the net's read-out set */
    int batch, rows, cols, classes; /* rows = cols = 0 for a ragged set */
    int64_t count;                  /* the pixels of all maps */
    int topk;                       /* 0, or the k of a top-k call: the maps are plane 0 of k rank-major planes, */
    int64_t plane_stride;           /* this many elements apart */
    /* which read-out geometry turned net->seg.dense_logits into the maps (mbn_net_segment_nll reads the logits again): the whole map or the
     * letterbox rectangle of a uniform call (the factor path: the whole map at out = factor x map, bit-equal), the net's ragged set, or several
     * presentations of an image (views, slide), which no single read-out of the logits reproduces */
    int geometry;                   /* MBN_SEG_GEOM_* */
    int32_t rect[4];                /* MBN_SEG_GEOM_RECT: (x, y, iw, ih) of the network input */
};
enum { MBN_SEG_GEOM_WHOLE = 0, MBN_SEG_GEOM_RECT = 1, MBN_SEG_GEOM_SET = 2, MBN_SEG_GEOM_MANY = 3 };

/* the segmentation state of a net: everything here is made on first use and freed by mbn_net_seg_release */
struct mbn_net_seg {
    void *dense_logits;             /* [max_batch][h][w][classes] fp32: the dense head's output, what every read-out reads */
    void *resize_buf;               /* the staging buffer: [max_batch][rows][cols][3] uint8, the resized images of every resize call */
    int resize_filter;              /* mbn_net_set_resize_filter: MBN_FILTER_* of every resizer (MBN_FILTER_BILINEAR until it is called) */
    uint8_t pad_color[3];           /* mbn_net_set_pad_color: the border of MBN_FIT_PAD, R, G, B (black until it is called) */
    mbn_resizer *resizer;           /* mbn_net_resize_input: the resizer of the geometry below, rebuilt when it changes */
    int rs_rows, rs_cols, rs_fit, rs_filter; float rs_fraction;
    uint8_t rs_color[3];            /* ... and the colour it was made for, when it is a letterbox */
    mbn_ragged_resizer *ragged;     /* the one ragged resizer of max_batch images (mbn_net_resize_inputs, _tiles), made for the key below */
    int ragged_filter, ragged_pad;  /* its filter; it is a letterbox handle (mbn_ragged_resizer_create_pad) */
    uint8_t ragged_color[3];        /* ... and then its colour */
    mbn_resize_item *ragged_items;  /* the items it is set from, [max_batch] */
    /* mbn_net_resize_views: the view resizers kept, each made for one (source size, scale, mirror, filter, pad colour); used = the clock of its last use */
    struct mbn_view_slot {
        mbn_resizer *r;
        int rows, cols, mirror, filter;
        float scale;
        uint8_t color[3];
        unsigned used;
    } view_cache[MBN_ENSEMBLE_MAX_VIEWS];
    unsigned view_clock;
    mbn_ragged_readout *readout;    /* mbn_net_segment_images: one ragged read-out of max_batch images */
    void *label_items;              /* ... and the items it is set from, [max_batch] mbn_label_window_item (or as many mbn_label_item) */
    struct mbn_seg_maps last;       /* the last successful segment call */
    mbn_components *components;     /* mbn_net_segment_regions: one handle, made again when a call needs more than it holds: */
    int components_batch;
    int64_t components_pixels;
    /* mbn_net_segment_panoptic: its handle and what it holds, the table size of both sides (mbn_net_set_panoptic_regions), and the buffers: both
     * segment maps and a widened uint8 truth ([panoptic_span] int32 each), both tables and both counts ([panoptic_batch] images) */
    mbn_panoptic *panoptic;
    int panoptic_batch, panoptic_regions, panoptic_max_regions;
    int64_t panoptic_span;
    void *panoptic_comp[2], *panoptic_wide, *panoptic_table[2], *panoptic_n[2];
    void *boundary_d;               /* mbn_net_segment_boundary_*: [max_batch] int32 on the device, the per-image half-widths of an image call */
    mbn_surface *surface;           /* mbn_net_segment_surface: one handle, made again when a call needs more than it holds: */
    int surface_batch, surface_classes;
    int64_t surface_pixels;
};

struct mbn_net {
    mbn_context *ctx;
    mbn_plan plan;
    int max_batch;
    int num_cus;               /* compute units of the context's GPU (small-batch fusion rule) */
    void *dev_blob;
    int own_blob;
    void *act[2];
    int keep;
    int dtype;                 /* MBN_DT_F32, MBN_DT_BF16 or MBN_DT_I8 */
    int fuse_stem;             /* mbn_net_set_fuse_stem (default 1) */
    int input_u8;              /* mbn_net_set_input_u8: images are raw uint8 HWC */
    unsigned fuse_blocks;      /* mbn_net_set_fuse_blocks: bit L = run the depthwise layer L and the pointwise layer L+1 as one launch */
    int fuse_blocks_set;       /* the caller chose a mask; otherwise the default of the current dtype applies */
    int use_graph;             /* mbn_net_set_graph */
    void *graph;               /* instantiated hipGraph of one forward, valid for the key below */
    int g_emul;                /* pw_emul value the graph was captured under */
    const void *g_images;
    void *g_logits;
    int g_batch, g_last, g_dtype, g_keep;
    int free_running;          /* no fork dependency on the context's stream (mbn_net_set_free_running) */
    const void *fr_images;     /* free-running: the (images, logits, batch, last_layer) of the previous forward; a call that */
    void *fr_logits;           /* differs re-inserts the fork wait, because sub-batch slices of act[] move with the batch */
    int fr_batch, fr_last, fr_ns, fr_stagger;
    int nstreams;              /* sub-batch pipelining (mbn_net_set_streams); 1 = everything on the context's stream */
    void *streams[8];
    void *bf16_filt[MBN_MAX_LAYERS];   /* bf16 copies of the pointwise / FC filters (bf16 mode) */
    unsigned char bf16_packed[MBN_MAX_LAYERS];   /* the copy is followed by its packed image (mbn_pack_filter_bf16) */
    void *keep_buf[MBN_MAX_LAYERS];
    void *logits_buf;          /* mbn_net_classify: [max_batch][classes] fp32 */
    void *dense_feat;          /* mbn_net_forward_dense: the activation in front of the pool, [max_batch][h][w][channels] at fp32 size */
    void *poolfc_ws;           /* workspace of mbn_pool_fc (1...4 images: pool + FC in one launch), allocated and zeroed at creation */
    size_t poolfc_ws_bytes;
    int fuse_tail;             /* mbn_net_set_fuse_tail (default 0) */
    int fuse_resident;         /* mbn_net_set_fuse_resident (default 1): runs of equal bf16 blocks on a small map as one launch, the map resident in LDS */
    void *last_out[MBN_MAX_LAYERS];
    /* I8 mode (mbn_quantize_i8): the quantized blob on the device, its layout, the activation scales it was made with, and the
     * host copy of the fp32 blob it is quantized from (downloaded once) */
    void *i8_blob;
    mbn_i8_params i8;
    float act_scale[MBN_MAX_LAYERS];
    float *host_blob;
    struct mbn_net_seg seg;    /* mbn_net_segment.c */
};

int mbn_net_dense_layers(const mbn_net *net, const mbn_layer_desc **feat, const mbn_layer_desc **fc);
void mbn_net_seg_release(mbn_net *net);    /* frees everything net->seg holds; mbn_net_destroy calls it with the device idle */

#endif
