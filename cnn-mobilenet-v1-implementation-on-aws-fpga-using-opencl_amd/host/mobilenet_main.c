/*
 * mobilenet_main.c — command-line C host; the counterpart of the reference's ./out (MobileNet.c main, :113-2833).
 *
 *   mobilenet --h5 weights.h5 [--ppm image.ppm] [--batch N] [--res 224] [--alpha 1.0]      fp32 path
 *   mobilenet --synthetic SEED [--alpha A] [--res R] [--batch N]                              fp32, synthetic weights
 *   --res R = R x R images; --res RxC = R rows by C columns (a P6 image C wide and R high), both multiples of 32
 *   --output-stride 32 | 16 | 8: the late stride-2 depthwise layers stop subsampling, the ones behind them are dilated (mbn_plan_build_os)
 *   --ppm F (several times, up to --batch, for files of different sizes: they are resized in ONE ragged launch, mbn_net_resize_inputs, and the top-1 of
 *   each is printed; the rest of the batch repeats the first): a P6 image of ANY size up to 8192 x 8192; one that is not cols wide and rows high is resized on the device (mbn_net_resize_input: Pillow's 8-bit
 *   bilinear). --fit crop (default: the centred box with the plan's aspect ratio) | stretch (the whole image); --crop-fraction F in (0, 1] shrinks the crop box
 *   (0.875 = "resize to 256, crop 224") | pad (the whole image with its aspect ratio kept, centred on a canvas of --pad-color R,G,B, default 0,0,0:
 *   PIL.ImageOps.pad, mbn_fit_pad; --segment then also prints the rectangle of image 0, which is where its labels are). An image of the plan's size
 *   is taken as it is
 *   --filter nearest | box | bilinear (default) | hamming | bicubic | lanczos: Pillow's filter of that resize (mbn_net_set_resize_filter). Several --ppm
 *   take the ragged launch, which has no hamming and no lanczos (their weights need the host's sin / cos): usage status 2
 *   --segment FILE: after the classification, the dense head (mbn_net_segment): the label map of image 0 as a binary PGM and its five most frequent labels
 *   --segment-source FILE: the label map of image 0 at that --ppm file's OWN width x height (needs --ppm and --fit stretch or --fit pad, else usage
 *   status 2: a crop has no labels for the rest of the image). stretch: one --ppm goes through mbn_net_resize_input + mbn_net_segment_to, several
 *   through mbn_net_segment_images (one ragged resize, one ragged read-out); pad: mbn_net_segment_fit / mbn_net_segment_images_fit, the read-out of
 *   the letterbox's rectangle, so the image is labelled undistorted
 *   --segment-confidence FILE: the softmax probability of the winning class at every pixel of image 0, at its own size, as an 8-bit PGM, byte =
 *   floor(prob * 255 + 0.5) (mbn_net_segment_prob_fit / _images_fit); valid wherever --segment-source is, with or without it
 *   --min-confidence P --ignore-label L (together, with --segment-source; P in [0, 1], L in 0..65535): the pixels of that label map whose probability
 *   is below P hold L instead of their label
 *   --segment-topk K (with ONE --ppm and --segment-source; 1 <= K <= 8): the K best classes of every pixel, mbn_net_segment_topk_fit. Rank 0 goes to
 *   the --segment-source file as without it, rank j >= 1 to out.rank<j>.pgm beside it (a slot no class filled is written as the value `classes`);
 *   with --segment-confidence conf.pgm every rank's probability likewise, conf.rank<j>.pgm; --min-confidence / --ignore-label act on rank 0 alone;
 *   with --truth ONE line: topk: k=K valid=... top1_acc=... top1_mean_acc=... ... topK_acc=... topK_mean_acc=... (mbn_topk_metrics). Not with
 *   --tta-scales, --slide, --regions, --panoptic or --boundary-*: usage status 2
 *   --tta-scales S1,S2,... [--tta-flip] (with ONE --ppm, --fit pad and --segment-source): test-time augmentation, mbn_net_segment_views_fit: the image
 *   is shown to the network at every scale (0 < S <= 1: the letterbox shrunk about the centre of the input), with --tta-flip also mirrored, and ONE
 *   read-out averages the views' logits. The views are (S1, plain), (S1, mirrored), (S2, plain), ... in that order, 8 at most (else usage status 2);
 *   --segment-confidence, --min-confidence and --ignore-label work as without it
 *   --slide TH[xTW] [--slide-stride SH[xSW]] (with ONE --ppm and --segment-source; rows x columns): sliding-window segmentation,
 *   mbn_net_segment_slide: overlapping TH x TW crops of the image, each stretched to the network's input, and ONE read-out that averages the crops'
 *   logits where they overlap. The default stride is (2 * tile + 2) / 3 per axis. The fit is the stretch: with --fit pad or --fit crop, or with
 *   --tta-scales / --tta-flip, usage status 2, as for a plan mbn_slide_plan refuses. --segment-confidence, --min-confidence, --ignore-label,
 *   --truth, --regions, --panoptic and --boundary-* work as without it
 *   --truth F.pgm (several times: the n-th pairs with the n-th --ppm, as many as there are; needs --segment-source): the ground truth of that image, a P5
 *   of its size (another size: error exit). maxval <= 255: one byte per pixel, uint8 truth; larger: two big-endian bytes, the format --segment-source
 *   itself writes, int32 truth, so a label map this tool wrote can be fed back. The label maps are scored on the device (mbn_net_segment_score: a value
 *   outside the classes is void in the truth and abstained in the labels, --ignore-label among them) and ONE line is printed:
 *   score: pixels=... valid=... void=... abstained=... classes_present=... pixel_acc=... mean_acc=... miou=... fw_iou=... (mbn_confusion_metrics, %.17g)
 *   --calibration BINS [--target-accuracy A] (with --segment-source, --segment-confidence and --truth; 1 <= BINS <= 1024, 0 <= A <= 1; else usage
 *   status 2): is the probability worth anything. The reliability table of the same maps and their probabilities, accumulated on the device
 *   (mbn_net_segment_calibration), and ONE line behind the score line (with --segment-topk: behind the topk line, for rank 0):
 *   calibration: bins=... answered=... abstained=... void=... accuracy=... mean_confidence=... ece=... mce=... aurc=...   (mbn_calibration_metrics)
 *   and with --target-accuracy, on the same line, the smallest --min-confidence whose kept pixels reach that accuracy (mbn_calibration_threshold):
 *   min_confidence=... coverage=... selective_accuracy=...  (min_confidence=none when no threshold of the table reaches it). With
 *   --min-confidence P > 0 the thresholded labels are what is scored: the pixels below P are in the abstained count and in no bin's accuracy.
 *   Works with --segment-topk, --tta-* and --slide like the other scores
 *   --nll [--temperatures T1,T2,...] (with --segment-source and --truth; up to 8 distinct T, each in [1/16, 16], default 1; else usage status 2; not
 *   with --segment-topk, --tta-* or --slide): are the probabilities worth anything as a whole. The NLL / Brier table of the softmax distribution of
 *   the same call at every temperature, read out again from the net's logits with the truth in the class loop (mbn_net_segment_nll); behind the
 *   calibration line one line per temperature, in descending T, and one for the best of them (mbn_nll_metrics, mbn_nll_best):
 *   nll: temperature=... scored=... void=... nll=... brier=... mean_class_nll=... accuracy=...
 *   nll_best: temperature=... refined_temperature=... at_edge=0|1   (temperature=none when nothing is scored)
 *   --regions [--connectivity 4|8] [--min-area N] [--max-regions M] (with --segment-source; defaults 4, 1, 256): the connected regions of every label
 *   map, found on the device (mbn_net_segment_regions). Per image one line `regions: image <n> count <k>` (k is the true count, even above M), then
 *   for each of its first min(k, M) regions `region <i> class <c> area <a> box <r0> <c0> <r1> <c1>` (rows first, both corners inside the box), in
 *   the order of the regions' first pixels. With --min-area N > 1 the regions of fewer than N pixels are dropped: the map written to --segment-source
 *   and the map scored by --truth are the cleaned ones, whose dropped pixels hold --ignore-label (where --min-confidence brought one), else the class
 *   count
 *   --panoptic [--connectivity 4|8] [--min-area N] (with --segment-source and --truth; defaults 4, 1): panoptic quality. The regions of every label
 *   map against the regions of its truth, both found on the device (mbn_net_segment_panoptic), at most 4096 a side. Behind the score line:
 *   panoptic: connectivity=... min_area=... scored=<images scored>/<images> classes_present=... tp=... fp=... fn=... pq=... sq=... rq=...
 *   panoptic_class: class <c> tp <n> fp <n> fn <n> pq <v> sq <v> rq <v>                               (one per present class)
 *   and, in front of them, `panoptic: image <n> not scored: ...` for an image with more regions than that on either side.
 *   --boundary-ratio R | --boundary-d N [--boundary-edge 0|1] [--boundary-map out.pgm] (with --segment-source; edge defaults to 1): contour quality,
 *   "score a segmentation at its boundaries" in mbn.h. The half-width is N pixels, or R of every image's own diagonal (0.02 is the usual value).
 *   With --truth three kinds of line follow the score line (mbn_net_segment_boundary_score):
 *   boundary: d=... edge=... classes_present=... truth_band=... pred_band=... boundary_miou=...      (d: image 0's half-width)
 *   boundary_iou: class <c> <iou>                                                                   (one per present class)
 *   trimap: ... the fields of the score line, over the pixels within d of a contour of the truth
 *   --boundary-map writes image 0's band as an 8-bit P5: byte = min (depth, d + 1) of its label map (mbn_net_segment_boundary_depth)
 *   --surface [--surface-bins N] [--surface-tolerance T] [--surface-percentile P] [--surface-edge 0|1] [--surface-map out.pgm] (with
 *   --segment-source and --truth; defaults 64, 2, 95, 1; else usage status 2, as for a bad value: 2 <= N <= 4096, 0 <= T <= N - 2, 0 < P <= 100):
 *   how far the predicted contours lie from the true ones, in pixels, "score a segmentation by surface distance" in mbn.h. Two kinds of line
 *   follow the other scores (mbn_net_segment_surface, mbn_surface_metrics):
 *   surface: bins=... tolerance=... percentile=... classes_present=... classes_measurable=... hd=... hdp=... assd=... nsd=... unmatched=... saturated=...
 *   surface_class: class <c> <hd> <hdp> <assd> <nsd>                                                (one per present class; nan where undefined)
 *   --surface-map writes image 0's contour as a 16-bit P5: 0 no contour pixel of a class, 65535 unmatched, else 1 + min (ceil (sqrt (d2)), 65533)
 *   mobilenet --literal [--weights weights_c.txt] [--image Cat_Image0.ppm] [--ref-args]      the reference's own mode
 *   mobilenet --gpus G --batch N [--steps K --warmup W --streams S --pw-emul 6] (--h5 F | --synthetic SEED)  N images sharded over G GPUs
 *   mobilenet --inspect weights.h5                                                             list the datasets of a .h5
 *   mobilenet --convert weights.h5 out.txt                                                     folded blob as text (one %.9g per line)
 *
 * --literal runs the 29 uint8/int32 layers exactly in MobileNet.c's order through the NULL-ext C-ABI calls, with the
 * reference's loaders (readSquezeNetKernel re-reads the same file prefix for every layer, decode_image keeps the PPM
 * header bytes). --ref-args additionally passes the reference's own argument literals where they differ from the
 * intended network (filtersize = K_P = 1 for pointwise, MobileNet.c:451; stride 2 at layer 26, :2432).
 * Prints the same two kinds of line as the reference: per-layer kernel time (MobileNet.c:315) and the argmax
 * line (MobileNet.c:2792).
 */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <unistd.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mbn.h"

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        int _rc = (call);                                                                             \
        if (_rc != MBN_OK) {                                                                          \
            fprintf(stderr, "Error: %s -> %s (%s)\n", #call, mbn_strerror(_rc),                       \
                    ctx ? mbn_last_device_error(ctx) : "");                                           \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

static int run_literal(mbn_context *ctx, const char *wfile, const char *image, int ref_args)
{
    mbn_plan plan;
    CHECK(mbn_plan_build(1.0f, 224, 1000, &plan));
    static unsigned char frame[224 * 224 * 3];
    unsigned char *r = malloc(224 * 224), *g = malloc(224 * 224), *b = malloc(224 * 224);
    int *filter = malloc(sizeof(int) * 1024 * 1024);
    if (!r || !g || !b || !filter) return 1;
    memset(frame, 0, sizeof(frame));
    if (decode_image(frame, (char *)image) != 0) fprintf(stderr, "warning: %s not readable; using a zero image\n", image);
    mbn_split_rgb(frame, 224 * 224, r, g, b);
    size_t act_bytes = 112 * 112 * 64;
    void *d_r, *d_g, *d_b, *d_f, *d_act[2];
    CHECK(mbn_alloc(ctx, 224 * 224, &d_r));
    CHECK(mbn_alloc(ctx, 224 * 224, &d_g));
    CHECK(mbn_alloc(ctx, 224 * 224, &d_b));
    CHECK(mbn_alloc(ctx, sizeof(int) * 1024 * 1024, &d_f));
    CHECK(mbn_alloc(ctx, act_bytes, &d_act[0]));
    CHECK(mbn_alloc(ctx, act_bytes, &d_act[1]));
    CHECK(mbn_upload(ctx, d_r, r, 224 * 224));
    CHECK(mbn_upload(ctx, d_g, g, 224 * 224));
    CHECK(mbn_upload(ctx, d_b, b, 224 * 224));
    CHECK(mbn_set_profiling(ctx, 1));
    const void *src = NULL;
    int which = 0;
    for (int i = 0; i < plan.n_layers; i++) {
        const mbn_layer_desc *l = &plan.layer[i];
        void *dst = d_act[which];
        int count = (int)l->w_count;
        if (l->kind != MBN_L_POOL) {
            memset(filter, 0, sizeof(int) * (size_t)count);
            int rc = mbn_read_text_weights(wfile, filter, count);     /* same prefix every layer, MobileNet.c:37 */
            if (rc != MBN_OK && i == 0) fprintf(stderr, "warning: %s: %s; missing weights read as 0\n", wfile, mbn_strerror(rc));
            CHECK(mbn_upload(ctx, d_f, filter, sizeof(int) * (size_t)count));
        }
        switch (l->kind) {
        case MBN_L_CONV:
            CHECK(mbn_convolute(ctx, dst, d_r, d_g, d_b, d_f, 224, 224, 3, 2, l->out_ch, NULL));
            break;
        case MBN_L_DW: {
            int stride = (ref_args && l->index == 26) ? 2 : l->stride;
            CHECK(mbn_depthwise(ctx, dst, src, d_f, l->out_rows, l->out_cols, 3, stride, l->out_ch, NULL));
            break;
        }
        case MBN_L_PW:
        case MBN_L_FC:
            CHECK(mbn_pointwise(ctx, dst, src, d_f, l->out_rows, l->out_cols, ref_args ? 1 : l->in_ch, l->out_ch, NULL));
            break;
        case MBN_L_POOL:
            CHECK(mbn_pool(ctx, dst, src, l->in_rows, l->in_cols, 7, l->out_ch, NULL));
            break;
        }
        float ms = 0.f;
        CHECK(mbn_last_kernel_ms(ctx, &ms));
        if (l->kind == MBN_L_FC) printf("Kernel Execution time for Fully Connected Layer: %f\n", ms / 1000.0);
        else printf("Kernel Execution time for Layer %d: %f\n", l->index, ms / 1000.0);
        src = dst;
        which ^= 1;
    }
    unsigned char logits[1000];
    double probs[1000], maximum;
    int location;
    CHECK(mbn_download(ctx, logits, src, 1000));
    mbn_softmax_argmax_u8(logits, 1000, probs, &location, &maximum);
    printf("Highest Probability of the element is present at location %d and it's value is %f.\n", location, maximum);
    free(r); free(g); free(b); free(filter);
    return 0;
}

static int inspect_cb(const char *path, int ndim, const int64_t *shape, void *user)
{
    long *total = (long *)user, n = 1;
    printf("%-56s (", path);
    for (int i = 0; i < ndim; i++) { printf(i ? ", %lld" : "%lld", (long long)shape[i]); n *= (long)shape[i]; }
    printf(")\n");
    *total += n;
    return 0;
}

/* Weight-format tooling (no GPU needed): what keras.py:1-8 was meant to do, done by parsing the HDF5 file. */
static int inspect_h5(const char *path)
{
    mbn_h5 *h5 = NULL;
    int rc = mbn_h5_open(path, &h5);
    if (rc != MBN_OK) { fprintf(stderr, "Error: %s: %s\n", path, mbn_strerror(rc)); return 1; }
    long total = 0;
    rc = mbn_h5_visit(h5, inspect_cb, &total);
    mbn_h5_close(h5);
    if (rc != MBN_OK) { fprintf(stderr, "Error: walking %s: %s\n", path, mbn_strerror(rc)); return 1; }
    printf("%ld float32 parameters\n", total);
    return 0;
}

static int convert_h5(const char *path, const char *out)
{
    mbn_weights w;
    int rc = mbn_weights_from_h5(path, 0.f, 224, &w);
    if (rc != MBN_OK) { fprintf(stderr, "Error: %s: %s\n", path, mbn_strerror(rc)); return 1; }
    FILE *fp = fopen(out, "w");
    if (!fp) { mbn_weights_free(&w); return 1; }
    fprintf(fp, "# mbn folded blob: alpha %g classes %d floats %lld\n", w.plan.alpha, w.plan.classes, (long long)w.plan.blob_floats);
    for (int64_t i = 0; i < w.plan.blob_floats; i++) fprintf(fp, "%.9g\n", w.blob[i]);
    fclose(fp);
    printf("alpha %g, %d classes, %lld floats -> %s\n", w.plan.alpha, w.plan.classes, (long long)w.plan.blob_floats, out);
    mbn_weights_free(&w);
    return 0;
}

/* ---------------------------------------------------------------------------------------------- --gpus G
 * The multi-GPU form of the host (BASELINE config 4): the batch is cut into G contiguous shards
 * (mbn_shard_range), GPU 0 receives the parameter blob from the host and ONE RCCL broadcast (mbn_dist_broadcast) hands it
 * to the other GPUs over xGMI, then one host thread per GPU runs the identical single-GPU pipeline on its shard. No
 * collective on the data path. Timing: W untimed steps, a thread barrier, K steps, device sync, barrier; the job's time
 * is the slowest GPU's (MAX), images/s = K * N / that. The reference drives exactly one device (MobileNet.c:155). */
typedef struct {
    int rank, world, batch, first, count, steps, warmup;
    mbn_dist *dist;
    const mbn_plan *plan;
    void *dev_blob;
    double seconds;
    int top1;            /* class of this shard's first image */
    float *logits;       /* host copy of the shard's logits after the timed steps [count][classes] (--verify, checksum) */
    unsigned long long fnv;
} gpu_job;

static double now_s(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static int g_streams = 1;      /* --streams S: sub-batch streams per GPU in --gpus mode (mbn_net_set_streams) */

/* image i of the whole batch is generated from its GLOBAL index, so a shard sees the same pixels as the same images would in
 * a single-GPU run (sharding property: concat of shards == the unsharded batch) */
static void synth_images(unsigned char *u8, int first, int n, size_t img)
{
    for (int i = 0; i < n; i++) {
        unsigned long long s = 0xC0FFEEULL + (unsigned long long)(first + i) * 0x9E3779B97F4A7C15ULL;
        unsigned char *p = u8 + (size_t)i * img;
        for (size_t k = 0; k < img; k++) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; p[k] = (unsigned char)(s >> 56); }
    }
}

static unsigned long long fnv1a(const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    unsigned long long h = 0xcbf29ce484222325ULL;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ULL; }
    return h;
}

/* the forward of images [first, first + n) on `ctx`, exactly as a rank runs it (same net settings, same call sizes): used by the
 * ranks and by --verify, which replays every shard on GPU 0 */
static int shard_forward(mbn_context *ctx, const mbn_plan *plan, void *dev_blob, int first, int n, int warmup, int steps,
                         float *host_logits, int *top1, double *seconds, mbn_rank_sync *sync)
{
    mbn_net *net = NULL;
    void *d_u8 = NULL, *d_logits = NULL, *d_idx = NULL, *d_prob = NULL;
    unsigned char *u8 = NULL;
    const int nn = n > 0 ? n : 1;                             /* a rank without images still takes part in the barriers */
    const size_t img = (size_t)plan->layer[0].in_rows * plan->layer[0].in_cols * 3;     /* [rows][cols][3] uint8 */
    int rc = mbn_net_create_from_device_blob(ctx, plan, dev_blob, nn, &net);
    if (rc == MBN_OK) rc = mbn_net_set_input_u8(net, 1);
    if (rc == MBN_OK && g_streams > 1) {
        rc = mbn_net_set_streams(net, g_streams);
        if (rc == MBN_OK) rc = mbn_net_set_free_running(net, 1);   /* the images are uploaded with the blocking mbn_upload below */
    }
    if (rc == MBN_OK) rc = mbn_alloc(ctx, (size_t)nn * img, &d_u8);
    if (rc == MBN_OK) rc = mbn_alloc(ctx, (size_t)nn * plan->classes * sizeof(float), &d_logits);
    if (rc == MBN_OK) rc = mbn_alloc(ctx, sizeof(int) * (size_t)nn, &d_idx);
    if (rc == MBN_OK) rc = mbn_alloc(ctx, sizeof(float) * (size_t)nn, &d_prob);
    if (rc == MBN_OK && !(u8 = malloc((size_t)nn * img))) rc = MBN_ENOMEM;
    if (rc == MBN_OK) {
        synth_images(u8, first, nn, img);
        rc = mbn_upload(ctx, d_u8, u8, (size_t)nn * img);
    }
    for (int w = 0; rc == MBN_OK && w < warmup && n > 0; w++) rc = mbn_net_forward(net, d_u8, d_logits, nn, 0);
    if (rc == MBN_OK) rc = mbn_sync(ctx);
    if (sync && (rc != MBN_OK ? (mbn_rank_fail(sync), 1) : mbn_rank_barrier(sync) != MBN_OK)) rc = rc != MBN_OK ? rc : MBN_EDEVICE;
    const double t0 = now_s();
    for (int k = 0; rc == MBN_OK && k < steps && n > 0; k++) rc = mbn_net_forward(net, d_u8, d_logits, nn, 0);
    if (rc == MBN_OK) rc = mbn_sync(ctx);
    if (seconds) *seconds = now_s() - t0;
    if (sync && rc == MBN_OK && mbn_rank_barrier(sync) != MBN_OK) rc = MBN_EDEVICE;
    if (rc == MBN_OK && n > 0) {
        int idx = -1;
        rc = mbn_softmax_topk_f32(ctx, NULL, d_idx, d_prob, d_logits, nn, plan->classes, 1, NULL);
        if (rc == MBN_OK) rc = mbn_download(ctx, &idx, d_idx, sizeof(int));
        if (top1) *top1 = idx + 1;
        if (rc == MBN_OK && host_logits) rc = mbn_download(ctx, host_logits, d_logits, (size_t)n * plan->classes * sizeof(float));
    }
    if (net) mbn_net_destroy(net);
    if (d_u8) mbn_free(ctx, d_u8);
    if (d_logits) mbn_free(ctx, d_logits);
    if (d_idx) mbn_free(ctx, d_idx);
    if (d_prob) mbn_free(ctx, d_prob);
    free(u8);
    return rc;
}

static int gpu_rank(int rank, void *arg, mbn_rank_sync *sync)
{
    gpu_job *j = &((gpu_job *)arg)[rank];
    mbn_context *ctx = NULL;
    int rc = mbn_dist_context(j->dist, j->rank, &ctx);
    if (rc == MBN_OK)
        rc = shard_forward(ctx, j->plan, j->dev_blob, j->first, j->count, j->warmup, j->steps, j->logits, &j->top1, &j->seconds, sync);
    if (rc == MBN_OK && j->count > 0) j->fnv = fnv1a(j->logits, (size_t)j->count * j->plan->classes * sizeof(float));
    if (rc != MBN_OK) fprintf(stderr, "Error: GPU %d: %s (%s)\n", j->rank, mbn_strerror(rc), ctx ? mbn_last_device_error(ctx) : "");
    return rc;
}

/* --gpus G [--verify]. Every failure leaves through `done`, which shuts the communicators and contexts down. */
static int run_multi(int gpus, int batch, int steps, int warmup, const mbn_weights *w, int verify)
{
    mbn_context *ctx = NULL;
    mbn_dist *dist = NULL;
    int bad = 1;
    int rc = mbn_dist_init(gpus, NULL, &dist);
    if (rc != MBN_OK) {
        fprintf(stderr, "Error: mbn_dist_init(%d) -> %s%s\n", gpus, mbn_strerror(rc),
                rc == MBN_ENODEVICE ? " (MBN_ENODEVICE: --gpus asks for more GPUs than this node shows)" : "");
        return 1;
    }
    const size_t blob_bytes = (size_t)w->plan.blob_floats * sizeof(float);
    void **blobs = calloc((size_t)gpus, sizeof(void *));
    gpu_job *jobs = calloc((size_t)gpus, sizeof(gpu_job));
    if (!blobs || !jobs) goto done;
#define TRY(call) do { rc = (call); if (rc != MBN_OK) { fprintf(stderr, "Error: %s -> %s (%s)\n", #call, mbn_strerror(rc), ctx ? mbn_last_device_error(ctx) : ""); goto done; } } while (0)
    for (int r = 0; r < gpus; r++) {
        TRY(mbn_dist_context(dist, r, &ctx));
        TRY(mbn_alloc(ctx, blob_bytes, &blobs[r]));
    }
    TRY(mbn_dist_context(dist, 0, &ctx));
    TRY(mbn_upload(ctx, blobs[0], w->blob, blob_bytes));        /* host -> GPU 0 once ... */
    rc = mbn_dist_broadcast(dist, blobs, blob_bytes, 0);         /* ... GPU 0 -> everybody over xGMI: the path's one collective */
    if (rc != MBN_OK) { fprintf(stderr, "Error: mbn_dist_broadcast -> %s (%s)\n", mbn_strerror(rc), mbn_dist_last_error(dist)); goto done; }
    for (int r = 0; r < gpus; r++) {
        gpu_job *j = &jobs[r];
        j->rank = r; j->world = gpus; j->batch = batch; j->steps = steps; j->warmup = warmup;
        j->dist = dist; j->plan = &w->plan; j->dev_blob = blobs[r];
        TRY(mbn_shard_range(batch, gpus, r, &j->first, &j->count));
        j->logits = malloc((size_t)(j->count > 0 ? j->count : 1) * w->plan.classes * sizeof(float));
        if (!j->logits) goto done;
    }
    rc = mbn_run_ranks(gpus, gpu_rank, jobs, -1, NULL);          /* one thread per GPU, gate + cancellable barrier (mbn_ranks.c) */
    if (rc != MBN_OK) { fprintf(stderr, "Error: a rank failed: %s\n", mbn_strerror(rc)); goto done; }
    double worst = 0.0;
    for (int r = 0; r < gpus; r++)
        if (jobs[r].seconds > worst) worst = jobs[r].seconds;
    for (int r = 0; r < gpus; r++)
        printf("GPU %d: images [%d, %d) %d steps in %.6f s; first image -> class %d; logits fnv1a %016llx\n", r, jobs[r].first,
               jobs[r].first + jobs[r].count, steps, jobs[r].seconds, jobs[r].top1, jobs[r].fnv);
    printf("%d GPUs, batch %d (%s), %d steps: %.1f images/sec (slowest GPU %.6f s, %.3f ms/step)\n", gpus, batch,
           "contiguous shards, weights broadcast once over RCCL", steps, (double)steps * batch / worst, worst,
           1000.0 * worst / steps);
    bad = 0;
    if (verify) {
        /* every shard again on GPU 0 — same images (global index), same call size, GPU 0's own copy of the blob — compared bit for
         * bit with what the shard's GPU produced: a wrong broadcast, a wrong shard offset or a GPU that computes differently shows */
        int differ = 0;
        bad = 1;                                                /* until every shard has compared identical (a failed TRY below left 0) */
        TRY(mbn_dist_context(dist, 0, &ctx));
        for (int r = 0; r < gpus; r++) {
            if (jobs[r].count <= 0) continue;
            const size_t nb = (size_t)jobs[r].count * w->plan.classes * sizeof(float);
            float *again = malloc(nb);
            if (!again) goto done;
            rc = shard_forward(ctx, &w->plan, blobs[0], jobs[r].first, jobs[r].count, 0, 1, again, NULL, NULL, NULL);
            const int same = rc == MBN_OK && memcmp(again, jobs[r].logits, nb) == 0;
            printf("verify: shard %d (GPU %d) vs the same images on GPU 0: %s (fnv1a %016llx)\n", r, r,
                   rc != MBN_OK ? mbn_strerror(rc) : same ? "identical" : "DIFFERENT", rc == MBN_OK ? fnv1a(again, nb) : 0ULL);
            free(again);
            if (!same) differ = 1;
        }
        bad = differ;
    }
#undef TRY
done:
    if (jobs)
        for (int r = 0; r < gpus; r++) free(jobs[r].logits);
    mbn_dist_shutdown(dist);                                    /* frees every buffer the contexts own, the communicators and the contexts */
    free(blobs); free(jobs);
    return bad;
}

/* --segment: image 0's label map [rows][cols] as a binary PGM (P5), maxval = max(classes - 1, 1), two big-endian bytes per pixel beyond 255;
 * then one line with the (at most) five most frequent labels, 0-based, and their pixel counts, most frequent first (ties: lowest label).
 * ignore >= 0 (--ignore-label, or the label of the pixels --min-area dropped): a pixel that holds it is written as it is and counted apart (`why`
 * says for what); maxval then covers it too */
static int write_label_map(const char *path, const int *labels, int rows, int cols, int classes, int ignore, const char *why)
{
    const int top = classes - 1 > ignore ? classes - 1 : ignore, maxval = top > 1 ? top : 1, wide = maxval > 255;
    long ignored = 0;
    FILE *fp = fopen(path, "wb");
    long *count = calloc((size_t)classes, sizeof(long));
    if (!fp || !count) { if (fp) fclose(fp); free(count); fprintf(stderr, "Error: cannot write %s\n", path); return 1; }
    fprintf(fp, "P5\n%d %d\n%d\n", cols, rows, maxval);
    for (long i = 0; i < (long)rows * cols; i++) {
        const int skip = ignore >= 0 && labels[i] == ignore;
        const int v = skip ? ignore : labels[i] < 0 ? 0 : labels[i] >= classes ? classes - 1 : labels[i];
        if (skip) ignored++;
        else count[v]++;
        if (wide) fputc(v >> 8, fp);
        fputc(v & 255, fp);
    }
    const int bad = fclose(fp) != 0;
    printf("segment: %dx%d label map -> %s; most frequent labels:", cols, rows, path);
    for (int j = 0; j < 5; j++) {
        int best = -1;
        for (int c = 0; c < classes; c++)
            if (count[c] > 0 && (best < 0 || count[c] > count[best])) best = c;
        if (best < 0) break;
        printf(" %d (%ld)", best, count[best]);
        count[best] = 0;
    }
    if (ignore >= 0) printf("; %s: %ld pixels, label %d", why, ignored, ignore);
    printf("\n");
    free(count);
    return bad;
}

/* width and height of a P6 file from its header (whitespace and # comments between the fields), so that the image buffer can be sized before
 * mbn_read_ppm fills it. MBN_OK, MBN_EIO or MBN_EFORMAT */
static int ppm_size(const char *path, int *width, int *height)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) return MBN_EIO;
    int ok = fgetc(fp) == 'P' && fgetc(fp) == '6', v[2] = { 0, 0 };
    for (int f = 0; ok && f < 2; f++) {
        int c = fgetc(fp);
        while (c == '#' || c == ' ' || c == '\t' || c == '\n' || c == '\r') {
            if (c == '#') while (c != '\n' && c != EOF) c = fgetc(fp);
            c = fgetc(fp);
        }
        int digits = 0;
        for (; c >= '0' && c <= '9' && digits < 6; c = fgetc(fp), digits++) v[f] = v[f] * 10 + (c - '0');
        ok = digits > 0 && digits < 6 && v[f] > 0;
    }
    fclose(fp);
    if (!ok) return MBN_EFORMAT;
    *width = v[0];
    *height = v[1];
    return MBN_OK;
}

#define PPM_MAX_SIDE 8192     /* the resize front-end's largest source side */

/* --truth: a P5 of exactly width x height into out [height * width]; maxval <= 255: a byte per pixel, else two big-endian bytes. *wide: maxval > 255.
 * 0, or 2 with a message for a file that is not such a P5 or has another size */
static int read_truth_pgm(const char *path, int width, int height, int32_t *out, int *wide)
{
    FILE *fp = fopen(path, "rb");
    int v[3] = { 0, 0, 0 };
    int ok = fp && fgetc(fp) == 'P' && fgetc(fp) == '5';
    for (int f = 0; ok && f < 3; f++) {
        int c = fgetc(fp);
        while (c == '#' || c == ' ' || c == '\t' || c == '\n' || c == '\r') {
            if (c == '#') while (c != '\n' && c != EOF) c = fgetc(fp);
            c = fgetc(fp);
        }
        int digits = 0;
        for (; c >= '0' && c <= '9' && digits < 6; c = fgetc(fp), digits++) v[f] = v[f] * 10 + (c - '0');
        ok = digits > 0 && digits < 6 && v[f] > 0 && (f < 2 || (v[f] <= 65535 && (c == ' ' || c == '\t' || c == '\n' || c == '\r')));
    }
    if (!ok) { if (fp) fclose(fp); fprintf(stderr, "--truth %s is not a readable P5 image\n", path); return 2; }
    if (v[0] != width || v[1] != height) {
        fclose(fp);
        fprintf(stderr, "--truth %s is %d x %d, its image %d x %d\n", path, v[0], v[1], width, height);
        return 2;
    }
    *wide = v[2] > 255;
    for (long i = 0; ok && i < (long)width * height; i++) {
        const int hi = *wide ? fgetc(fp) : 0, lo = fgetc(fp);
        ok = hi != EOF && lo != EOF;
        out[i] = (hi << 8) | lo;
    }
    fclose(fp);
    if (!ok) { fprintf(stderr, "--truth %s ends before its last pixel\n", path); return 2; }
    return 0;
}

/* --boundary-ratio / --boundary-d / --boundary-edge / --boundary-map: what the command line asked for; on = 0: nothing. d > 0: a fixed half-width,
 * else `ratio` of every image's diagonal */
typedef struct boundary_opts { int on, d, edge; double ratio; const char *map; } boundary_opts;

/* --truth with --boundary-ratio or --boundary-d: the boundary IoU and the trimap scores of the same maps (mbn_net_segment_boundary_score) */
static int score_boundary(mbn_context *ctx, mbn_net *net, const boundary_opts *bo, void *d_labels, void *d_truth, int tb, int classes, int rows0, int cols0)
{
    const size_t cells = ((size_t)classes + 1) * ((size_t)classes + 1), bcells = (size_t)classes * 3;
    uint64_t *trimap = malloc(cells * sizeof(uint64_t)), *biou = malloc(bcells * sizeof(uint64_t));
    double *iou = malloc((size_t)classes * sizeof(double));
    if (!trimap || !biou || !iou) return 1;
    void *d_trimap, *d_biou;
    CHECK(mbn_alloc(ctx, cells * sizeof(uint64_t), &d_trimap));
    CHECK(mbn_alloc(ctx, bcells * sizeof(uint64_t), &d_biou));
    CHECK(mbn_memset(ctx, d_trimap, 0, cells * sizeof(uint64_t)));
    CHECK(mbn_memset(ctx, d_biou, 0, bcells * sizeof(uint64_t)));
    CHECK(mbn_net_segment_boundary_score(net, d_labels, d_truth, tb, d_trimap, d_biou, bo->ratio, bo->d, bo->edge));
    CHECK(mbn_download(ctx, trimap, d_trimap, cells * sizeof(uint64_t)));
    CHECK(mbn_download(ctx, biou, d_biou, bcells * sizeof(uint64_t)));
    CHECK(mbn_free(ctx, d_trimap));
    CHECK(mbn_free(ctx, d_biou));
    mbn_boundary_metrics_t b;
    mbn_seg_metrics m;
    CHECK(mbn_boundary_metrics(biou, classes, &b, iou));
    printf("boundary: d=%d edge=%d classes_present=%d truth_band=%.0f pred_band=%.0f boundary_miou=%.17g\n",
           bo->d > 0 ? bo->d : mbn_boundary_d(rows0, cols0, bo->ratio), bo->edge, b.classes_present, b.truth_band_pixels, b.pred_band_pixels, b.boundary_miou);
    for (int c = 0; c < classes; c++)
        if (!isnan(iou[c])) printf("boundary_iou: class %d %.17g\n", c, iou[c]);
    CHECK(mbn_confusion_metrics(trimap, classes, &m, NULL));
    printf("trimap: pixels=%.0f valid=%.0f void=%.0f abstained=%.0f classes_present=%d pixel_acc=%.17g mean_acc=%.17g miou=%.17g fw_iou=%.17g\n", m.pixels,
           m.valid, m.void_pixels, m.abstained, m.classes_present, m.pixel_accuracy, m.mean_accuracy, m.miou, m.fw_iou);
    free(trimap); free(biou); free(iou);
    return 0;
}

/* --boundary-map: image 0's band, the depth min (D, d + 1) of its label map as an 8-bit P5 (mbn_net_segment_boundary_depth) */
static int write_boundary_map(mbn_context *ctx, mbn_net *net, const boundary_opts *bo, void *d_labels, size_t pixels, int rows, int cols)
{
    unsigned char *depth = malloc((size_t)rows * cols);
    if (!depth) return 1;
    void *d_depth;
    CHECK(mbn_alloc(ctx, pixels, &d_depth));
    CHECK(mbn_net_segment_boundary_depth(net, d_labels, d_depth, bo->ratio, bo->d, bo->edge));
    CHECK(mbn_download(ctx, depth, d_depth, (size_t)rows * cols));       /* image 0 is first in the buffer */
    CHECK(mbn_free(ctx, d_depth));
    FILE *fp = fopen(bo->map, "wb");
    if (!fp) { fprintf(stderr, "Error: cannot write %s\n", bo->map); return 1; }
    fprintf(fp, "P5\n%d %d\n255\n", cols, rows);
    const int d = bo->d > 0 ? bo->d : mbn_boundary_d(rows, cols, bo->ratio);
    long band = 0;
    for (long i = 0; i < (long)rows * cols; i++) band += depth[i] <= d;
    const int ok = fwrite(depth, 1, (size_t)rows * cols, fp) == (size_t)rows * cols;
    printf("boundary-map: %dx%d -> %s; d=%d, %ld pixels in the band\n", cols, rows, bo->map, d, band);
    free(depth);
    return (fclose(fp) != 0) | !ok;
}

/* --panoptic [--connectivity 4|8] [--min-area N]: what the command line asked for; on = 0: nothing */
typedef struct panoptic_opts { int on, connectivity, min_area; } panoptic_opts;

/* --truth with --panoptic: the regions of the same maps against the regions of the truth (mbn_net_segment_panoptic) */
static int panoptic_table(mbn_context *ctx, mbn_net *net, const panoptic_opts *po, int n, void *d_labels, void *d_truth, int tb, size_t cells,
                          void *d_pq, void *d_scored, uint64_t *pq, int32_t *scored)
{
    CHECK(mbn_memset(ctx, d_pq, 0, cells * sizeof(uint64_t)));
    CHECK(mbn_net_segment_panoptic(net, d_labels, d_truth, tb, po->connectivity, po->min_area, d_pq, d_scored));
    CHECK(mbn_download(ctx, pq, d_pq, cells * sizeof(uint64_t)));
    CHECK(mbn_download(ctx, scored, d_scored, (size_t)n * sizeof(int32_t)));
    return 0;
}

static int score_panoptic(mbn_context *ctx, mbn_net *net, const panoptic_opts *po, int n, void *d_labels, void *d_truth, int tb, int classes)
{
    const size_t cells = (size_t)classes * 4;
    uint64_t *pq = malloc(cells * sizeof(uint64_t));
    int32_t *scored = malloc((size_t)n * sizeof(int32_t));
    double *per = malloc(3 * (size_t)classes * sizeof(double));
    void *d_pq = NULL, *d_scored = NULL;
    int bad = !pq || !scored || !per;
    if (!bad && (mbn_alloc(ctx, cells * sizeof(uint64_t), &d_pq) != MBN_OK || mbn_alloc(ctx, (size_t)n * sizeof(int32_t), &d_scored) != MBN_OK)) {
        fprintf(stderr, "Error: --panoptic: no device memory for its table (%s)\n", mbn_last_device_error(ctx));
        bad = 1;
    }
    if (!bad) bad = panoptic_table(ctx, net, po, n, d_labels, d_truth, tb, cells, d_pq, d_scored, pq, scored);
    if (d_pq) mbn_free(ctx, d_pq);
    if (d_scored) mbn_free(ctx, d_scored);
    if (bad) {
        free(pq); free(scored); free(per);
        return 1;
    }
    int images = 0;
    for (int i = 0; i < n; i++) {
        images += scored[i] != 0;
        if (!scored[i]) printf("panoptic: image %d not scored: more than %d regions on one side\n", i, MBN_NET_PANOPTIC_REGIONS);
    }
    mbn_panoptic_metrics_t m;
    if (mbn_panoptic_metrics(pq, classes, &m, per, per + classes, per + 2 * classes) != MBN_OK) {
        free(pq); free(scored); free(per);
        return 1;
    }
    printf("panoptic: connectivity=%d min_area=%d scored=%d/%d classes_present=%d tp=%.0f fp=%.0f fn=%.0f pq=%.17g sq=%.17g rq=%.17g\n", po->connectivity,
           po->min_area, images, n, m.classes_present, m.tp, m.fp, m.fn, m.pq, m.sq, m.rq);
    for (int c = 0; c < classes; c++)
        if (!isnan(per[c]))
            printf("panoptic_class: class %d tp %llu fp %llu fn %llu pq %.17g sq %.17g rq %.17g\n", c, (unsigned long long)pq[4 * c],
                   (unsigned long long)pq[4 * c + 1], (unsigned long long)pq[4 * c + 2], per[c], per[classes + c], per[2 * classes + c]);
    free(pq); free(scored); free(per);
    return 0;
}

/* --calibration BINS [--target-accuracy A]: what the command line asked for; bins = 0: nothing (like g_streams, set once by main) */
static struct { int bins, have_target; double target; } g_calibration = { 0, 0, 0.0 };

/* --truth with --calibration: the reliability table of the same maps and their probabilities at d_prob (mbn_net_segment_calibration), ONE line */
static int score_calibration(mbn_context *ctx, mbn_net *net, void *d_labels, void *d_prob, void *d_truth, int tb)
{
    const int bins = g_calibration.bins;
    const size_t bytes = ((size_t)bins + 1) * 4 * sizeof(uint64_t);
    uint64_t *calib = malloc(bytes);
    if (!calib) return 1;
    void *d_calib;
    CHECK(mbn_alloc(ctx, bytes, &d_calib));
    CHECK(mbn_memset(ctx, d_calib, 0, bytes));
    CHECK(mbn_net_segment_calibration(net, d_labels, d_prob, d_truth, tb, bins, d_calib));
    CHECK(mbn_download(ctx, calib, d_calib, bytes));
    CHECK(mbn_free(ctx, d_calib));
    mbn_calibration m;
    CHECK(mbn_calibration_metrics(calib, bins, &m, NULL, NULL, NULL, NULL));
    printf("calibration: bins=%d answered=%.0f abstained=%.0f void=%.0f accuracy=%.17g mean_confidence=%.17g ece=%.17g mce=%.17g aurc=%.17g", bins,
           m.answered, m.abstained, m.void_pixels, m.accuracy, m.mean_confidence, m.ece, m.mce, m.aurc);
    if (g_calibration.have_target) {
        float min_prob = 0.0f;
        double coverage = 0.0, selective = 0.0;
        const int rc = mbn_calibration_threshold(calib, bins, g_calibration.target, &min_prob, &coverage, &selective);
        if (rc == MBN_OK) printf(" min_confidence=%.9g coverage=%.17g selective_accuracy=%.17g", (double)min_prob, coverage, selective);
        else if (rc == MBN_ENOTFOUND) printf(" min_confidence=none coverage=0 selective_accuracy=nan");      /* no edge reaches the target */
        else CHECK(rc);
    }
    printf("\n");
    free(calib);
    return 0;
}

/* --nll [--temperatures T1,T2,...]: what the command line asked for; temps = 0: nothing (set once by main). inv[j] = 1 / T_j, ascending */
static struct { int temps; float temperature[MBN_NLL_MAX_TEMPS], inv[MBN_NLL_MAX_TEMPS]; } g_nll = { 0, { 0 }, { 0 } };

/* --temperatures: up to MBN_NLL_MAX_TEMPS comma-separated T, each with 1 / T in [1/16, 16]; kept in descending T, so that 1 / T ascends as
 * mbn_nll_best asks. 0 on success */
static int parse_temperatures(const char *s)
{
    int n = 0;
    while (*s) {
        char *end;
        const double t = strtod(s, &end);
        if (end == s || n == MBN_NLL_MAX_TEMPS || !(t >= 0.0625 && t <= 16.0) || (*end && *end != ',')) return 1;
        g_nll.temperature[n++] = (float)t;
        s = *end ? end + 1 : end;
        if (*end && !*s) return 1;                               /* a trailing comma */
    }
    for (int i = 1; i < n; i++)                                  /* insertion sort, T descending; equal temperatures are refused */
        for (int j = i; j > 0 && g_nll.temperature[j] > g_nll.temperature[j - 1]; j--) {
            const float v = g_nll.temperature[j];
            g_nll.temperature[j] = g_nll.temperature[j - 1];
            g_nll.temperature[j - 1] = v;
        }
    for (int i = 0; i < n; i++) {
        g_nll.inv[i] = 1.0f / g_nll.temperature[i];
        if (i > 0 && !(g_nll.inv[i] > g_nll.inv[i - 1])) return 1;
    }
    g_nll.temps = n;
    return n == 0;
}

/* --truth with --nll: the NLL / Brier table of the probabilities of the same call, read out again from the net's logits (mbn_net_segment_nll):
 * one nll: line per temperature and one nll_best: line */
static int score_nll(mbn_context *ctx, mbn_net *net, void *d_truth, int tb, int classes, size_t pixels)
{
    const int temps = g_nll.temps;
    const size_t bytes = (size_t)temps * ((size_t)classes + 1) * 4 * sizeof(uint64_t);
    uint64_t *table = malloc(bytes);
    if (!table) return 1;
    void *d_table;
    CHECK(mbn_alloc(ctx, bytes, &d_table));
    CHECK(mbn_memset(ctx, d_table, 0, bytes));
    CHECK(mbn_net_segment_nll(net, d_truth, tb, g_nll.inv, temps, d_table, NULL, NULL, (int64_t)pixels));
    CHECK(mbn_download(ctx, table, d_table, bytes));
    CHECK(mbn_free(ctx, d_table));
    for (int j = 0; j < temps; j++) {
        mbn_nll m;
        CHECK(mbn_nll_metrics(table, classes, temps, j, &m, NULL, NULL));
        printf("nll: temperature=%.9g scored=%.0f void=%.0f nll=%.17g brier=%.17g mean_class_nll=%.17g accuracy=%.17g\n", (double)g_nll.temperature[j],
               m.scored, m.void_pixels, m.nll, m.brier, m.mean_class_nll, m.accuracy);
    }
    int best = 0, at_edge = 0;
    double inv = 0.0;
    const int rc = mbn_nll_best(table, classes, temps, g_nll.inv, &best, &inv, &at_edge);
    if (rc == MBN_OK) printf("nll_best: temperature=%.9g refined_temperature=%.17g at_edge=%d\n", (double)g_nll.temperature[best], 1.0 / inv, at_edge);
    else if (rc == MBN_ENOTFOUND) printf("nll_best: temperature=none refined_temperature=nan at_edge=0\n");      /* nothing scored */
    else CHECK(rc);
    free(table);
    return 0;
}

/* --surface [--surface-bins N] [--surface-tolerance T] [--surface-percentile P] [--surface-edge 0|1] [--surface-map out.pgm]: what the command line
 * asked for; on = 0: nothing (set once by main) */
static struct { int on, bins, tolerance, edge; double percentile; const char *map; } g_surface = { 0, 64, 2, 1, 95.0, NULL };

/* the smallest t with t * t >= d2 (d2 < 2^31) */
static unsigned ceil_root(unsigned d2)
{
    unsigned t = (unsigned)sqrt((double)d2);
    while ((uint64_t)t * t > d2) t--;
    while ((uint64_t)(t + 1) * (t + 1) <= d2) t++;
    return t + ((uint64_t)t * t < d2);
}

/* --truth with --surface: the surface-distance table of the same maps (mbn_net_segment_surface), the surface: line and one surface_class: line per
 * present class; --surface-map: image 0's contour (at element first, rows x cols) as a 16-bit P5 of its distances */
static int score_surface(mbn_context *ctx, mbn_net *net, void *d_labels, void *d_truth, int tb, int classes, size_t pixels, int64_t first, int rows,
                         int cols)
{
    const int bins = g_surface.bins;
    const size_t cells = (size_t)classes * 2 * (MBN_SURFACE_HEAD + (size_t)bins);
    uint64_t *surf = malloc(cells * sizeof(uint64_t));
    double *per = malloc(4 * (size_t)classes * sizeof(double));
    uint32_t *d2 = g_surface.map ? malloc((size_t)rows * cols * sizeof(uint32_t)) : NULL;
    if (!surf || !per || (g_surface.map && !d2)) return 1;
    void *d_surf, *d_d2 = NULL;
    CHECK(mbn_alloc(ctx, cells * sizeof(uint64_t), &d_surf));
    if (g_surface.map) CHECK(mbn_alloc(ctx, pixels * sizeof(uint32_t), &d_d2));
    CHECK(mbn_memset(ctx, d_surf, 0, cells * sizeof(uint64_t)));
    CHECK(mbn_net_segment_surface(net, d_labels, d_truth, tb, bins, g_surface.edge, d_surf, d_d2));
    CHECK(mbn_download(ctx, surf, d_surf, cells * sizeof(uint64_t)));
    CHECK(mbn_free(ctx, d_surf));
    mbn_surface_metrics_t m;
    CHECK(mbn_surface_metrics(surf, classes, bins, g_surface.tolerance, g_surface.percentile, &m, per, per + classes, per + 2 * classes, per + 3 * classes));
    printf("surface: bins=%d tolerance=%d percentile=%.17g classes_present=%d classes_measurable=%d hd=%.17g hdp=%.17g assd=%.17g nsd=%.17g unmatched=%.0f "
           "saturated=%d\n", bins, g_surface.tolerance, g_surface.percentile, m.classes_present, m.classes_measurable, m.hd, m.hdp, m.assd, m.nsd, m.unmatched,
           m.saturated);
    for (int c = 0; c < classes; c++)
        if (!isnan(per[3 * classes + c]))
            printf("surface_class: class %d %.17g %.17g %.17g %.17g\n", c, per[c], per[classes + c], per[2 * classes + c], per[3 * classes + c]);
    free(surf); free(per);
    if (!g_surface.map) return 0;
    CHECK(mbn_download(ctx, d2, (const char *)d_d2 + (size_t)first * sizeof(uint32_t), (size_t)rows * cols * sizeof(uint32_t)));
    CHECK(mbn_free(ctx, d_d2));
    FILE *fp = fopen(g_surface.map, "wb");
    if (!fp) { fprintf(stderr, "Error: cannot write %s\n", g_surface.map); return 1; }
    fprintf(fp, "P5\n%d %d\n65535\n", cols, rows);
    long queries = 0;
    int ok = 1;
    for (long i = 0; i < (long)rows * cols; i++) {
        /* not a query: 0; unmatched: 65535; matched: 1 + min (ceil (sqrt (d2)), 65533) */
        unsigned v = 0;
        if (d2[i] == 0xFFFFFFFEu) v = 65535;
        else if (d2[i] != 0xFFFFFFFFu) { const unsigned t = ceil_root(d2[i]); v = 1 + (t < 65533 ? t : 65533); }
        queries += v != 0;
        const unsigned char be[2] = { (unsigned char)(v >> 8), (unsigned char)(v & 255) };
        ok &= fwrite(be, 1, 2, fp) == 2;
    }
    printf("surface-map: %dx%d -> %s; %ld contour pixels\n", cols, rows, g_surface.map, queries);
    free(d2);
    return (fclose(fp) != 0) | !ok;
}

/* --truth: scores the label maps the segment call just wrote at d_labels (image n at element dst[n]) against the files, and prints the line;
 * --calibration (d_prob: the probabilities of the same call): the calibration line behind it; bo->on: the boundary lines behind that; po->on: the
 * panoptic lines behind those */
static int score_truth(mbn_context *ctx, mbn_net *net, const char **truths, int n, const int64_t *dst, const int32_t *hs, const int32_t *ws, size_t pixels,
                       void *d_labels, void *d_prob, int classes, const boundary_opts *bo, const panoptic_opts *po)
{
    int32_t *tv = calloc(pixels, sizeof(int32_t));
    if (!tv) return 1;
    int any_wide = 0;
    for (int i = 0; i < n; i++) {
        int wide = 0;
        const int bad = read_truth_pgm(truths[i], ws[i], hs[i], tv + dst[i], &wide);
        if (bad) return bad;
        any_wide |= wide;
    }
    unsigned char *t8 = NULL;
    if (!any_wide) {                                            /* every file has a byte per pixel: uint8 truth */
        t8 = malloc(pixels);
        if (!t8) return 1;
        for (size_t i = 0; i < pixels; i++) t8[i] = (unsigned char)tv[i];
    }
    const int tb = any_wide ? 4 : 1;
    const size_t cells = ((size_t)classes + 1) * ((size_t)classes + 1);
    uint64_t *counts = malloc(cells * sizeof(uint64_t));
    double *iou = malloc((size_t)classes * sizeof(double));
    if (!counts || !iou) return 1;
    void *d_truth, *d_counts;
    CHECK(mbn_alloc(ctx, pixels * (size_t)tb, &d_truth));
    CHECK(mbn_alloc(ctx, cells * sizeof(uint64_t), &d_counts));
    CHECK(mbn_upload(ctx, d_truth, any_wide ? (const void *)tv : (const void *)t8, pixels * (size_t)tb));
    CHECK(mbn_memset(ctx, d_counts, 0, cells * sizeof(uint64_t)));
    CHECK(mbn_net_segment_score(net, d_labels, d_truth, tb, d_counts));
    CHECK(mbn_download(ctx, counts, d_counts, cells * sizeof(uint64_t)));
    CHECK(mbn_free(ctx, d_counts));
    mbn_seg_metrics m;
    CHECK(mbn_confusion_metrics(counts, classes, &m, iou));
    printf("score: pixels=%.0f valid=%.0f void=%.0f abstained=%.0f classes_present=%d pixel_acc=%.17g mean_acc=%.17g miou=%.17g fw_iou=%.17g\n", m.pixels,
           m.valid, m.void_pixels, m.abstained, m.classes_present, m.pixel_accuracy, m.mean_accuracy, m.miou, m.fw_iou);
    if (g_calibration.bins) {
        const int bad = score_calibration(ctx, net, d_labels, d_prob, d_truth, tb);
        if (bad) return bad;
    }
    if (g_nll.temps) {
        const int bad = score_nll(ctx, net, d_truth, tb, classes, pixels);
        if (bad) return bad;
    }
    if (bo->on) {
        const int bad = score_boundary(ctx, net, bo, d_labels, d_truth, tb, classes, hs[0], ws[0]);
        if (bad) return bad;
    }
    if (po->on) {
        const int bad = score_panoptic(ctx, net, po, n, d_labels, d_truth, tb, classes);
        if (bad) return bad;
    }
    if (g_surface.on) {
        const int bad = score_surface(ctx, net, d_labels, d_truth, tb, classes, pixels, dst[0], hs[0], ws[0]);
        if (bad) return bad;
    }
    CHECK(mbn_free(ctx, d_truth));
    free(tv); free(t8); free(counts); free(iou);
    return 0;
}

/* --regions: what the command line asked for; on = 0: nothing */
typedef struct region_opts { int on, connectivity, min_area, max_regions; } region_opts;

/* --regions: the regions of the label maps the segment call just wrote at d_labels (n images), printed; *d_clean: with --min-area > 1 a new buffer
 * with the cleaned maps at the same offsets (dropped pixels hold `ignore`), else NULL */
static int print_regions(mbn_context *ctx, mbn_net *net, const region_opts *ro, int n, size_t pixels, void *d_labels, int ignore, void **d_clean)
{
    const size_t cap = (size_t)ro->max_regions;
    mbn_region *table = malloc((cap ? cap : 1) * (size_t)n * sizeof(mbn_region));
    int32_t *count = malloc((size_t)n * sizeof(int32_t));
    if (!table || !count) return 1;
    void *d_table = NULL, *d_count;
    *d_clean = NULL;
    if (cap) CHECK(mbn_alloc(ctx, cap * (size_t)n * sizeof(mbn_region), &d_table));
    CHECK(mbn_alloc(ctx, (size_t)n * sizeof(int32_t), &d_count));
    if (ro->min_area > 1) CHECK(mbn_alloc(ctx, pixels * sizeof(int32_t), d_clean));
    CHECK(mbn_net_segment_regions(net, d_labels, NULL, (mbn_region *)d_table, d_count, *d_clean, ro->connectivity, ro->min_area, ignore, ro->max_regions));
    CHECK(mbn_download(ctx, count, d_count, (size_t)n * sizeof(int32_t)));
    if (cap) CHECK(mbn_download(ctx, table, d_table, cap * (size_t)n * sizeof(mbn_region)));
    for (int i = 0; i < n; i++) {
        printf("regions: image %d count %d\n", i, count[i]);
        for (size_t k = 0; k < cap && k < (size_t)count[i]; k++) {
            const mbn_region *g = &table[(size_t)i * cap + k];
            printf("region %zu class %d area %d box %d %d %d %d\n", k, g->label, g->area, g->min_row, g->min_col, g->max_row, g->max_col);
        }
    }
    if (d_table) CHECK(mbn_free(ctx, d_table));
    CHECK(mbn_free(ctx, d_count));
    free(table); free(count);
    return 0;
}

/* --segment-confidence: image 0's probability map [rows][cols] as an 8-bit P5, byte = floor(prob * 255 + 0.5) */
static int write_confidence_map(const char *path, const float *prob, int rows, int cols)
{
    FILE *fp = fopen(path, "wb");
    if (!fp) { fprintf(stderr, "Error: cannot write %s\n", path); return 1; }
    fprintf(fp, "P5\n%d %d\n255\n", cols, rows);
    double sum = 0.0;
    for (long i = 0; i < (long)rows * cols; i++) {
        fputc((int)floor((double)prob[i] * 255.0 + 0.5), fp);      /* exact in double: no build rounds it another way */
        sum += prob[i];
    }
    printf("segment: %dx%d confidence map -> %s; mean probability %.4f\n", cols, rows, path, sum / ((double)rows * cols));
    return fclose(fp) != 0;
}

/* --segment-source: the --ppm files again, at their own sizes, one behind the other in ONE device buffer; image 0's label map at its own size.
 * One file: mbn_net_resize_input (stretch) + mbn_net_segment_to; several: mbn_net_segment_images. Under --fit pad mbn_net_segment_fit /
 * mbn_net_segment_images_fit, the read-out through the letterbox. The net takes uint8 images (the caller has set that).
 * conf_path (--segment-confidence) or ignore >= 0 (--min-confidence with --ignore-label): the softmax read-out instead, mbn_net_segment_prob_fit /
 * mbn_net_segment_prob_images_fit: image 0's probability map as an 8-bit P5, byte = floor(prob * 255 + 0.5), and the label map with the pixels
 * below min_conf replaced by `ignore`. path may then be NULL (no label map asked for).
 * n_views > 0 (--tta-scales; one file, --fit pad): mbn_net_segment_views_fit over the views (scales[k], mirrors[k]) instead, either read-out.
 * slide (--slide; one file): mbn_net_segment_slide with the tile slide[0] x slide[1] at the stride slide[2] x slide[3] instead, either read-out.
 * ro->on (--regions): the regions of every map are printed first; with --min-area > 1 the cleaned maps take the place of the maps from there on.
 * n_truth > 0 (--truth, one per image): the maps are scored against them on the device before anything is written */
static int segment_source(mbn_context *ctx, mbn_net *net, const char **ppms, int n_ppm, const char *path, int classes, int fit, const char *conf_path,
                          float min_conf, int ignore, const float *scales, const int32_t *mirrors, int n_views, const int *slide, const char **truths,
                          int n_truth, const region_opts *ro, const boundary_opts *bo, const panoptic_opts *po)
{
    int64_t *offs = malloc(sizeof(int64_t) * (size_t)n_ppm), *dst = malloc(sizeof(int64_t) * (size_t)n_ppm);
    int32_t *hs = malloc(sizeof(int32_t) * (size_t)n_ppm), *ws = malloc(sizeof(int32_t) * (size_t)n_ppm);
    if (!offs || !dst || !hs || !ws) return 1;
    size_t total = 0, pixels = 0;
    for (int n = 0; n < n_ppm; n++) {
        int pw = 0, ph = 0;
        if (ppm_size(ppms[n], &pw, &ph) != MBN_OK || pw > PPM_MAX_SIDE || ph > PPM_MAX_SIDE) {
            fprintf(stderr, "%s is not a readable P6 image of at most %d x %d pixels\n", ppms[n], PPM_MAX_SIDE, PPM_MAX_SIDE);
            return 2;
        }
        offs[n] = (int64_t)total; dst[n] = (int64_t)pixels; hs[n] = ph; ws[n] = pw;
        total += (size_t)pw * ph * 3;
        pixels += (size_t)pw * ph;
    }
    unsigned char *all = malloc(total);
    int *labels = malloc(sizeof(int) * (size_t)hs[0] * ws[0]);
    if (!all || !labels) return 1;
    for (int n = 0; n < n_ppm; n++) {
        int pw = ws[n], ph = hs[n];
        if (mbn_read_ppm(ppms[n], all + offs[n], &pw, &ph, pw * ph) != MBN_OK) { fprintf(stderr, "cannot read %s\n", ppms[n]); return 2; }
    }
    void *d_src, *d_img, *d_labels, *d_prob = NULL;
    CHECK(mbn_alloc(ctx, total, &d_src));
    CHECK(mbn_alloc(ctx, sizeof(int) * pixels, &d_labels));
    CHECK(mbn_upload(ctx, d_src, all, total));
    if (!(min_conf > 0.0f)) ignore = -1;                        /* --min-confidence 0 replaces nothing: the argmax read-out, unless a map is asked for */
    if (slide) {
        if (conf_path) CHECK(mbn_alloc(ctx, sizeof(float) * pixels, &d_prob));
        CHECK(mbn_net_segment_slide(net, d_src, 1, hs[0], ws[0], slide[0], slide[1], slide[2], slide[3], d_labels, d_prob, NULL,
                                    ignore >= 0 ? min_conf : 0.0f, ignore >= 0 ? ignore : 0));
        printf("segment: tiles of %d x %d at a stride of %d x %d (rows x columns) averaged in one read-out\n", slide[0], slide[1], slide[2], slide[3]);
    } else if (n_views > 0) {
        if (conf_path) CHECK(mbn_alloc(ctx, sizeof(float) * pixels, &d_prob));
        CHECK(mbn_net_segment_views_fit(net, d_src, 1, hs[0], ws[0], scales, mirrors, n_views, d_labels, d_prob, NULL, ignore >= 0 ? min_conf : 0.0f,
                                        ignore >= 0 ? ignore : 0));
        printf("segment: %d views averaged in one read-out\n", n_views);
    } else if (conf_path || ignore >= 0) {
        const float min_prob = ignore >= 0 ? min_conf : 0.0f;
        if (conf_path) CHECK(mbn_alloc(ctx, sizeof(float) * pixels, &d_prob));
        if (n_ppm == 1) CHECK(mbn_net_segment_prob_fit(net, d_src, 1, hs[0], ws[0], fit, d_labels, d_prob, min_prob, ignore));
        else CHECK(mbn_net_segment_prob_images_fit(net, d_src, offs, hs, ws, n_ppm, fit, d_labels, dst, d_prob, min_prob, ignore));
    } else if (fit == MBN_FIT_PAD) {
        if (n_ppm == 1) CHECK(mbn_net_segment_fit(net, d_src, 1, hs[0], ws[0], MBN_FIT_PAD, d_labels, NULL));
        else CHECK(mbn_net_segment_images_fit(net, d_src, offs, hs, ws, n_ppm, MBN_FIT_PAD, d_labels, dst, NULL));
    } else if (n_ppm == 1) {
        CHECK(mbn_net_resize_input(net, d_src, 1, hs[0], ws[0], MBN_FIT_STRETCH, 1.0f, &d_img));
        CHECK(mbn_net_segment_to(net, d_img, 1, hs[0], ws[0], d_labels, NULL));
    } else {
        CHECK(mbn_net_segment_images(net, d_src, offs, hs, ws, n_ppm, d_labels, dst, NULL));
    }
    int bad = 0;
    const char *why = "below --min-confidence";
    void *d_maps = d_labels, *d_clean = NULL;                   /* the maps that are scored and written */
    if (ro->on) {
        bad = print_regions(ctx, net, ro, n_ppm, pixels, d_labels, ignore >= 0 ? ignore : classes, &d_clean);
        if (bad) return bad;
        if (d_clean) {
            d_maps = d_clean;
            why = ignore >= 0 ? "below --min-confidence or --min-area" : "below --min-area";
            if (ignore < 0) ignore = classes;
        }
    }
    CHECK(mbn_download(ctx, labels, d_maps, sizeof(int) * (size_t)hs[0] * ws[0]));        /* image 0 is first in the buffer */
    if (n_truth > 0) {                                          /* the maps are where every path above wrote them: image n at element dst[n] */
        bad = score_truth(ctx, net, truths, n_truth, dst, hs, ws, pixels, d_maps, d_prob, classes, bo, po);
        if (bad) return bad;
    }
    if (bo->map) {
        bad = write_boundary_map(ctx, net, bo, d_maps, pixels, hs[0], ws[0]);
        if (bad) return bad;
    }
    if (d_clean) CHECK(mbn_free(ctx, d_clean));
    if (conf_path) {
        float *prob = malloc(sizeof(float) * (size_t)hs[0] * ws[0]);
        if (!prob) return 1;
        CHECK(mbn_download(ctx, prob, d_prob, sizeof(float) * (size_t)hs[0] * ws[0]));
        CHECK(mbn_free(ctx, d_prob));
        bad = write_confidence_map(conf_path, prob, hs[0], ws[0]);
        free(prob);
    }
    CHECK(mbn_free(ctx, d_src));
    CHECK(mbn_free(ctx, d_labels));
    if (path) bad |= write_label_map(path, labels, hs[0], ws[0], classes, ignore, why);
    free(all); free(labels); free(offs); free(dst); free(hs); free(ws);
    return bad;
}

/* path with ".rank<j>" in front of its extension (out.pgm -> out.rank2.pgm; no extension: behind the name) */
static void rank_path(char *out, size_t size, const char *path, int j)
{
    const char *slash = strrchr(path, '/'), *dot = strrchr(path, '.');
    if (!dot || (slash && dot < slash)) dot = path + strlen(path);
    snprintf(out, size, "%.*s.rank%d%s", (int)(dot - path), path, j, dot);
}

/* --segment-topk K (one --ppm, --fit stretch or pad, --segment-source): mbn_net_segment_topk_fit. Rank 0 goes to `path` as without it, rank j >= 1 to
 * out.rank<j>.pgm beside it (an unfilled slot, label -1, is written as the value `classes` and counted apart); with conf_path every rank's probability
 * map likewise; with a truth file ONE line with the top-1 .. top-K pixel accuracy and mean accuracy (mbn_net_segment_topk_score, mbn_topk_metrics).
 * min_conf / ignore act on rank 0 only, as in segment_source */
static int segment_source_topk(mbn_context *ctx, mbn_net *net, const char *ppm, const char *path, int classes, int fit, int k, const char *conf_path,
                               float min_conf, int ignore, const char *truth)
{
    int pw = 0, ph = 0;
    if (ppm_size(ppm, &pw, &ph) != MBN_OK || pw > PPM_MAX_SIDE || ph > PPM_MAX_SIDE) {
        fprintf(stderr, "%s is not a readable P6 image of at most %d x %d pixels\n", ppm, PPM_MAX_SIDE, PPM_MAX_SIDE);
        return 2;
    }
    const size_t pixels = (size_t)pw * ph;
    unsigned char *src = malloc(pixels * 3);
    int *labels = malloc(sizeof(int) * pixels * (size_t)k);
    if (!src || !labels) return 1;
    if (mbn_read_ppm(ppm, src, &pw, &ph, pw * ph) != MBN_OK) { fprintf(stderr, "cannot read %s\n", ppm); return 2; }
    if (!(min_conf > 0.0f)) ignore = -1;                        /* --min-confidence 0 replaces nothing */
    void *d_src, *d_labels, *d_prob = NULL;
    CHECK(mbn_alloc(ctx, pixels * 3, &d_src));
    CHECK(mbn_alloc(ctx, sizeof(int) * pixels * (size_t)k, &d_labels));
    if (conf_path) CHECK(mbn_alloc(ctx, sizeof(float) * pixels * (size_t)k, &d_prob));
    CHECK(mbn_upload(ctx, d_src, src, pixels * 3));
    CHECK(mbn_net_segment_topk_fit(net, d_src, 1, ph, pw, fit, k, d_labels, d_prob, NULL, ignore >= 0 ? min_conf : 0.0f, ignore >= 0 ? ignore : 0));
    if (truth) {
        int32_t *tv = calloc(pixels, sizeof(int32_t));
        const size_t cells = ((size_t)classes + 1) * ((size_t)k + 1);
        uint64_t *ranks = malloc(cells * sizeof(uint64_t));
        if (!tv || !ranks) return 1;
        int wide = 0;
        const int bad = read_truth_pgm(truth, pw, ph, tv, &wide);
        if (bad) return bad;
        void *d_truth, *d_ranks;
        CHECK(mbn_alloc(ctx, pixels * sizeof(int32_t), &d_truth));
        CHECK(mbn_alloc(ctx, cells * sizeof(uint64_t), &d_ranks));
        CHECK(mbn_upload(ctx, d_truth, tv, pixels * sizeof(int32_t)));                        /* int32 truth either way: a byte value is itself */
        CHECK(mbn_memset(ctx, d_ranks, 0, cells * sizeof(uint64_t)));
        CHECK(mbn_net_segment_topk_score(net, d_labels, d_truth, 4, d_ranks));
        CHECK(mbn_download(ctx, ranks, d_ranks, cells * sizeof(uint64_t)));
        CHECK(mbn_free(ctx, d_ranks));
        double acc[MBN_TOPK_MAX], mean[MBN_TOPK_MAX], valid = 0.0;
        CHECK(mbn_topk_metrics(ranks, classes, k, acc, mean, &valid));
        printf("topk: k=%d valid=%.0f", k, valid);
        for (int j = 0; j < k; j++) printf(" top%d_acc=%.17g top%d_mean_acc=%.17g", j + 1, acc[j], j + 1, mean[j]);
        printf("\n");
        if (g_calibration.bins) {                               /* plane 0 of the rank-major labels and probabilities is the map to score */
            const int bad_cal = score_calibration(ctx, net, d_labels, d_prob, d_truth, 4);
            if (bad_cal) return bad_cal;
        }
        CHECK(mbn_free(ctx, d_truth));
        free(tv); free(ranks);
    }
    CHECK(mbn_download(ctx, labels, d_labels, sizeof(int) * pixels * (size_t)k));
    int bad = write_label_map(path, labels, ph, pw, classes, ignore, "below --min-confidence");
    char name[4096];
    for (int j = 1; j < k && !bad; j++) {
        int *plane = labels + (size_t)j * pixels;
        for (size_t i = 0; i < pixels; i++)
            if (plane[i] < 0) plane[i] = classes;
        rank_path(name, sizeof name, path, j);
        bad = write_label_map(name, plane, ph, pw, classes, classes, "unfilled");
    }
    if (conf_path && !bad) {
        float *prob = malloc(sizeof(float) * pixels * (size_t)k);
        if (!prob) return 1;
        CHECK(mbn_download(ctx, prob, d_prob, sizeof(float) * pixels * (size_t)k));
        CHECK(mbn_free(ctx, d_prob));
        for (int j = 0; j < k && !bad; j++) {
            if (j) rank_path(name, sizeof name, conf_path, j);
            bad = write_confidence_map(j ? name : conf_path, prob + (size_t)j * pixels, ph, pw);
        }
        free(prob);
    }
    CHECK(mbn_free(ctx, d_src));
    CHECK(mbn_free(ctx, d_labels));
    free(src); free(labels);
    return bad;
}

/* --fit NAME: MBN_FIT_*, or -1 for an unknown name */
static int fit_of(const char *name)
{
    return !strcmp(name, "crop") ? MBN_FIT_CROP : !strcmp(name, "stretch") ? MBN_FIT_STRETCH : !strcmp(name, "pad") ? MBN_FIT_PAD : -1;
}

static const char *fit_name(int fit)
{
    return fit == MBN_FIT_CROP ? "crop" : fit == MBN_FIT_PAD ? "pad" : "stretch";
}

/* --pad-color R,G,B: three integers 0..255 and nothing behind them */
static int pad_color_of(const char *s, int rgb[3])
{
    char extra;
    if (sscanf(s, "%d,%d,%d%c", &rgb[0], &rgb[1], &rgb[2], &extra) != 3) return 0;
    return rgb[0] >= 0 && rgb[0] <= 255 && rgb[1] >= 0 && rgb[1] <= 255 && rgb[2] >= 0 && rgb[2] <= 255;
}

/* --slide TH[xTW] / --slide-stride SH[xSW]: rows, then columns (one number: both); positive integers and nothing else */
static int rows_cols_of(const char *s, int *r, int *c)
{
    char *end = NULL;
    const long a = strtol(s, &end, 10);
    long b = a;
    if (end == s) return 0;
    if (*end == 'x' || *end == 'X') {
        const char *t = end + 1;
        b = strtol(t, &end, 10);
        if (end == t) return 0;
    }
    if (*end || a < 1 || b < 1 || a > PPM_MAX_SIDE || b > PPM_MAX_SIDE) return 0;
    *r = (int)a; *c = (int)b;
    return 1;
}

/* --tta-scales S1,S2,...: up to MBN_ENSEMBLE_MAX_VIEWS numbers in (0, 1] and nothing else; their count, or 0 for anything else */
static int tta_scales_of(const char *s, float scales[MBN_ENSEMBLE_MAX_VIEWS])
{
    int n = 0;
    while (*s) {
        char *end;
        const float v = strtof(s, &end);
        if (end == s || n == MBN_ENSEMBLE_MAX_VIEWS || !(v > 0.0f) || !(v <= 1.0f)) return 0;
        scales[n++] = v;
        if (*end == ',' && end[1]) s = end + 1;
        else if (!*end) break;
        else return 0;
    }
    return n;
}

/* --filter NAME: MBN_FILTER_*, or -1 for an unknown name */
static int filter_of(const char *name)
{
    static const char *const names[] = { "nearest", "lanczos", "bilinear", "bicubic", "box", "hamming" };      /* MBN_FILTER_* order */
    for (int f = 0; f < 6; f++)
        if (!strcmp(name, names[f])) return f;
    return -1;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "--inspect")) return inspect_h5(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "--convert")) return convert_h5(argv[2], argv[3]);
    const char **ppms = malloc(sizeof(char *) * (size_t)argc);          /* every --ppm, in order */
    const char **truths = malloc(sizeof(char *) * (size_t)argc);        /* every --truth, in order */
    int n_ppm = 0, n_truth = 0;
    if (!ppms || !truths) return 1;
    const char *h5 = NULL, *ppm = NULL, *segment = NULL, *segment_src = NULL, *segment_conf = NULL, *wfile = "weights_c.txt", *image = "Cat_Image0.ppm";
    int fit = MBN_FIT_CROP, filter = MBN_FILTER_BILINEAR;
    int pad_rgb[3] = { 0, 0, 0 }, src_h0 = 0, src_w0 = 0;              /* src_h0 x src_w0: image 0 as it was resized (0: it was not) */
    float crop_fraction = 1.0f, min_conf = 0.0f;
    int have_min_conf = 0, have_ignore = 0, ignore_label = -1, have_topk = 0, segment_topk = 0, have_calibration = 0, calibration_bins = 0, have_nll = 0;
    const char *temperatures = NULL;
    const char *tta = NULL, *slide_arg = NULL, *slide_stride_arg = NULL;
    int fit_given = 0, slide[4] = { 0, 0, 0, 0 }, slide_tiles = 0;      /* slide: tile rows, tile columns, stride rows, stride columns */
    region_opts regions = { 0, 4, 1, 256 };
    int region_flags = 0;                                       /* --connectivity, --min-area or --max-regions seen */
    int max_regions_flag = 0;                                   /* --max-regions seen: it belongs to --regions alone */
    panoptic_opts panoptic = { 0, 4, 1 };
    boundary_opts boundary = { 0, 0, 1, 0.0, NULL };
    int boundary_flags = 0;                                     /* --boundary-edge seen */
    int surface_on = 0, surface_flags = 0;                      /* --surface, one of its options */
    int tta_flip = 0, n_views = 0;
    float tta_scales[MBN_ENSEMBLE_MAX_VIEWS], view_scales[MBN_ENSEMBLE_MAX_VIEWS];
    int32_t view_mirrors[MBN_ENSEMBLE_MAX_VIEWS];
    int literal = 0, ref_args = 0, batch = 1, rows = 224, cols = 224, have_seed = 0, gpus = 0, steps = 20, warmup = 3, verify = 0, out_stride = 32;
    unsigned long long seed = 0;
    float alpha = 0.f;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--h5") && i + 1 < argc) h5 = argv[++i];
        else if (!strcmp(argv[i], "--ppm") && i + 1 < argc) ppms[n_ppm++] = argv[++i];
        else if (!strcmp(argv[i], "--weights") && i + 1 < argc) wfile = argv[++i];
        else if (!strcmp(argv[i], "--image") && i + 1 < argc) image = argv[++i];
        else if (!strcmp(argv[i], "--batch") && i + 1 < argc) batch = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--res") && i + 1 < argc) {          /* R or RxC, rows first */
            const char *r = argv[++i];
            char *end = NULL;
            rows = cols = (int)strtol(r, &end, 10);
            if (end && (*end == 'x' || *end == 'X')) cols = atoi(end + 1);
        }
        else if (!strcmp(argv[i], "--alpha") && i + 1 < argc) alpha = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--output-stride") && i + 1 < argc) out_stride = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--segment") && i + 1 < argc) segment = argv[++i];
        else if (!strcmp(argv[i], "--segment-source") && i + 1 < argc) segment_src = argv[++i];
        else if (!strcmp(argv[i], "--segment-confidence") && i + 1 < argc) segment_conf = argv[++i];
        else if (!strcmp(argv[i], "--segment-topk") && i + 1 < argc) { segment_topk = atoi(argv[++i]); have_topk = 1; }
        else if (!strcmp(argv[i], "--min-confidence") && i + 1 < argc) { min_conf = (float)atof(argv[++i]); have_min_conf = 1; }
        else if (!strcmp(argv[i], "--ignore-label") && i + 1 < argc) { ignore_label = atoi(argv[++i]); have_ignore = 1; }
        else if (!strcmp(argv[i], "--tta-scales") && i + 1 < argc) tta = argv[++i];
        else if (!strcmp(argv[i], "--tta-flip")) tta_flip = 1;
        else if (!strcmp(argv[i], "--slide") && i + 1 < argc) slide_arg = argv[++i];
        else if (!strcmp(argv[i], "--slide-stride") && i + 1 < argc) slide_stride_arg = argv[++i];
        else if (!strcmp(argv[i], "--truth") && i + 1 < argc) truths[n_truth++] = argv[++i];
        else if (!strcmp(argv[i], "--calibration") && i + 1 < argc) { calibration_bins = atoi(argv[++i]); have_calibration = 1; }
        else if (!strcmp(argv[i], "--target-accuracy") && i + 1 < argc) { g_calibration.target = atof(argv[++i]); g_calibration.have_target = 1; }
        else if (!strcmp(argv[i], "--nll")) have_nll = 1;
        else if (!strcmp(argv[i], "--temperatures") && i + 1 < argc) temperatures = argv[++i];
        else if (!strcmp(argv[i], "--regions")) regions.on = 1;
        else if (!strcmp(argv[i], "--panoptic")) panoptic.on = 1;
        else if (!strcmp(argv[i], "--boundary-ratio") && i + 1 < argc) { boundary.ratio = atof(argv[++i]); boundary.on |= 1; }
        else if (!strcmp(argv[i], "--boundary-d") && i + 1 < argc) { boundary.d = atoi(argv[++i]); boundary.on |= 2; }
        else if (!strcmp(argv[i], "--boundary-edge") && i + 1 < argc) { boundary.edge = atoi(argv[++i]); boundary_flags = 1; }
        else if (!strcmp(argv[i], "--boundary-map") && i + 1 < argc) boundary.map = argv[++i];
        else if (!strcmp(argv[i], "--surface")) surface_on = 1;
        else if (!strcmp(argv[i], "--surface-bins") && i + 1 < argc) { g_surface.bins = atoi(argv[++i]); surface_flags = 1; }
        else if (!strcmp(argv[i], "--surface-tolerance") && i + 1 < argc) { g_surface.tolerance = atoi(argv[++i]); surface_flags = 1; }
        else if (!strcmp(argv[i], "--surface-percentile") && i + 1 < argc) { g_surface.percentile = atof(argv[++i]); surface_flags = 1; }
        else if (!strcmp(argv[i], "--surface-edge") && i + 1 < argc) { g_surface.edge = atoi(argv[++i]); surface_flags = 1; }
        else if (!strcmp(argv[i], "--surface-map") && i + 1 < argc) { g_surface.map = argv[++i]; surface_flags = 1; }
        else if (!strcmp(argv[i], "--connectivity") && i + 1 < argc) { regions.connectivity = atoi(argv[++i]); region_flags = 1; }
        else if (!strcmp(argv[i], "--min-area") && i + 1 < argc) { regions.min_area = atoi(argv[++i]); region_flags = 1; }
        else if (!strcmp(argv[i], "--max-regions") && i + 1 < argc) { regions.max_regions = atoi(argv[++i]); region_flags = max_regions_flag = 1; }
        else if (!strcmp(argv[i], "--fit") && i + 1 < argc && fit_of(argv[i + 1]) >= 0) { fit = fit_of(argv[++i]); fit_given = 1; }
        else if (!strcmp(argv[i], "--pad-color") && i + 1 < argc && pad_color_of(argv[i + 1], pad_rgb)) i++;
        else if (!strcmp(argv[i], "--crop-fraction") && i + 1 < argc) crop_fraction = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--filter") && i + 1 < argc && filter_of(argv[i + 1]) >= 0) filter = filter_of(argv[++i]);
        else if (!strcmp(argv[i], "--synthetic") && i + 1 < argc) { seed = strtoull(argv[++i], NULL, 0); have_seed = 1; }
        else if (!strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--steps") && i + 1 < argc) steps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--streams") && i + 1 < argc) g_streams = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--pw-emul") && i + 1 < argc) {          /* opt-in arithmetic form of the pointwise layers (mbn.h: pw_emul) */
            if (mbn_tune_set("pw_emul", atoi(argv[++i])) != MBN_OK || mbn_tune_set("pw_emul_static", 1) != MBN_OK) { fprintf(stderr, "bad --pw-emul\n"); return 2; }
        }
        else if (!strcmp(argv[i], "--warmup") && i + 1 < argc) warmup = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--verify")) verify = 1;
        else if (!strcmp(argv[i], "--literal")) literal = 1;
        else if (!strcmp(argv[i], "--ref-args")) ref_args = 1;
        else {
            fprintf(stderr, "usage: %s [--h5 F | --synthetic SEED | --literal] [--ppm F ... [--fit crop|stretch|pad] [--crop-fraction F] [--pad-color R,G,B] [--filter nearest|box|bilinear|hamming|bicubic|lanczos]] [--batch N] [--res R | RxC] [--alpha A] [--output-stride 32|16|8] [--segment OUT.pgm] [--segment-source OUT.pgm [--segment-topk K] [--min-confidence P --ignore-label L] [--tta-scales S1,S2,... [--tta-flip]] [--slide TH[xTW] [--slide-stride SH[xSW]]] [--truth F.pgm ...] [--calibration BINS [--target-accuracy A]] [--nll [--temperatures T1,T2,...]] [--regions [--connectivity 4|8] [--min-area N] [--max-regions M]] [--boundary-ratio R | --boundary-d N [--boundary-edge 0|1] [--boundary-map OUT.pgm]] [--panoptic [--connectivity 4|8] [--min-area N]] [--surface [--surface-bins N] [--surface-tolerance T] [--surface-percentile P] [--surface-edge 0|1] [--surface-map OUT.pgm]]] [--segment-confidence OUT.pgm] "
                            "[--gpus G [--steps K] [--warmup W] [--streams S] [--pw-emul 6] [--verify]]\n"
                            "  --calibration BINS [--target-accuracy A]: with --segment-confidence and --truth, one calibration: line (reliability table "
                            "in BINS bins, ECE, MCE, AURC) and the smallest --min-confidence that reaches accuracy A; with --min-confidence P > 0 the "
                            "thresholded labels are scored, the pixels below P count as abstained\n"
                            "  --nll [--temperatures T1,T2,...]: with --truth, one nll: line per temperature (NLL, Brier score, mean-class NLL of the softmax "
                            "distribution scaled by 1 / T; default 1) and one nll_best: line (the T with the smallest NLL, refined, at_edge)\n", argv[0]);
            return 2;
        }
    }
    if (!(crop_fraction > 0.f) || !(crop_fraction <= 1.f)) { fprintf(stderr, "bad --crop-fraction (0 < F <= 1)\n"); return 2; }
    if (n_ppm > 1 && n_ppm > batch) { fprintf(stderr, "%d --ppm files need --batch %d at least\n", n_ppm, n_ppm); return 2; }
    if (n_ppm > 1 && (filter == MBN_FILTER_HAMMING || filter == MBN_FILTER_LANCZOS)) {
        fprintf(stderr, "--filter %s with several --ppm: the ragged resize forms its weights on the device, which has no sin / cos bit-equal to the host's; "
                        "use nearest, box, bilinear or bicubic, or one --ppm\n", filter == MBN_FILTER_HAMMING ? "hamming" : "lanczos");
        return 2;
    }
    if (n_ppm == 1) ppm = ppms[0];
    if (slide_arg || slide_stride_arg) {
        /* sliding window: a tile is a crop of the source stretched to the input, so the fit is the stretch; the letterbox, the crop and the views
         * have no part in it */
        if (!slide_arg || !segment_src || n_ppm != 1 || (fit_given && fit != MBN_FIT_STRETCH) || tta || tta_flip ||
            !rows_cols_of(slide_arg, &slide[0], &slide[1]) || (slide_stride_arg && !rows_cols_of(slide_stride_arg, &slide[2], &slide[3]))) {
            fprintf(stderr, "--slide TH[xTW] [--slide-stride SH[xSW]] (rows x columns; the default stride is (2 * tile + 2) / 3) needs one --ppm and "
                            "--segment-source and goes with --fit stretch alone, not with --tta-scales / --tta-flip\n");
            return 2;
        }
        if (!slide_stride_arg) { slide[2] = (2 * slide[0] + 2) / 3; slide[3] = (2 * slide[1] + 2) / 3; }
        fit = MBN_FIT_STRETCH;
        int sw = 0, sh = 0;
        mbn_slide plan;
        if (ppm_size(ppm, &sw, &sh) != MBN_OK || sw > PPM_MAX_SIDE || sh > PPM_MAX_SIDE) {
            fprintf(stderr, "%s is not a readable P6 image of at most %d x %d pixels\n", ppm, PPM_MAX_SIDE, PPM_MAX_SIDE);
            return 2;
        }
        const int rc = mbn_slide_plan(sh, sw, slide[0], slide[1], slide[2], slide[3], &plan);
        if (rc != MBN_OK) {
            fprintf(stderr, "--slide %dx%d --slide-stride %dx%d on a %d x %d image (rows x columns): %s; a tile is at most the image, a stride between "
                            "half a tile and a tile, and an axis takes at most %d tiles\n", slide[0], slide[1], slide[2], slide[3], sh, sw,
                    mbn_strerror(rc), MBN_SLIDE_MAX_AXIS);
            return 2;
        }
        slide_tiles = plan.ny * plan.nx;                        /* the tiles of the image are one batch of the net */
    }
    if (segment_src && (n_ppm < 1 || (fit != MBN_FIT_STRETCH && fit != MBN_FIT_PAD))) {
        fprintf(stderr, "--segment-source needs --ppm and --fit stretch or --fit pad\n");
        return 2;
    }
    if (segment_conf && (n_ppm < 1 || (fit != MBN_FIT_STRETCH && fit != MBN_FIT_PAD))) {
        fprintf(stderr, "--segment-confidence needs --ppm and --fit stretch or --fit pad\n");
        return 2;
    }
    if (have_topk && (!segment_src || n_ppm != 1 || segment_topk < 1 || segment_topk > MBN_TOPK_MAX || tta || tta_flip || slide_arg || regions.on ||
                      panoptic.on || boundary.on || boundary.map)) {
        fprintf(stderr, "--segment-topk K (1 <= K <= %d) needs one --ppm and --segment-source with --fit stretch or --fit pad; it goes with "
                        "--segment-confidence, --min-confidence / --ignore-label and --truth, not with --tta-scales, --slide, --regions, --panoptic or "
                        "--boundary-*\n", MBN_TOPK_MAX);
        return 2;
    }
    if (tta || tta_flip) {
        const int n_scales = tta ? tta_scales_of(tta, tta_scales) : 0;
        if (!segment_src || fit != MBN_FIT_PAD || n_ppm != 1 || n_scales < 1 || n_scales * (1 + tta_flip) > MBN_ENSEMBLE_MAX_VIEWS) {
            fprintf(stderr, "--tta-scales S1,S2,... (each in (0, 1]; with --tta-flip twice as many views, %d at most) needs one --ppm, --fit pad and "
                            "--segment-source\n", MBN_ENSEMBLE_MAX_VIEWS);
            return 2;
        }
        for (int k = 0; k < n_scales; k++)
            for (int m = 0; m <= tta_flip; m++) { view_scales[n_views] = tta_scales[k]; view_mirrors[n_views++] = m; }
    }
    if (n_truth > 0 && (!segment_src || n_truth != n_ppm)) {
        fprintf(stderr, "--truth F.pgm needs --segment-source and comes once per --ppm, in the same order\n");
        return 2;
    }
    if (have_calibration || g_calibration.have_target) {
        if (!have_calibration || !segment_src || !segment_conf || n_truth == 0) {
            fprintf(stderr, "--calibration BINS [--target-accuracy A] needs --segment-source, --segment-confidence (the probabilities it scores) and "
                            "--truth; --target-accuracy needs --calibration\n");
            return 2;
        }
        if (calibration_bins < 1 || calibration_bins > MBN_CALIBRATION_MAX_BINS ||
            (g_calibration.have_target && !(g_calibration.target >= 0.0 && g_calibration.target <= 1.0))) {
            fprintf(stderr, "bad --calibration (1 <= BINS <= %d) or --target-accuracy (0 <= A <= 1)\n", MBN_CALIBRATION_MAX_BINS);
            return 2;
        }
        g_calibration.bins = calibration_bins;
    }
    if (have_nll || temperatures) {
        if (!have_nll || !segment_src || n_truth == 0 || have_topk || tta || tta_flip || slide_arg) {
            fprintf(stderr, "--nll [--temperatures T1,T2,...] needs --segment-source and --truth and does not go with --segment-topk, --tta-scales or "
                            "--slide (several presentations of an image are another probability model); --temperatures needs --nll\n");
            return 2;
        }
        if (parse_temperatures(temperatures ? temperatures : "1")) {
            fprintf(stderr, "bad --temperatures: 1 to %d distinct comma-separated values, each in [1/16, 16]\n", MBN_NLL_MAX_TEMPS);
            return 2;
        }
    }
    if (boundary.on || boundary_flags || boundary.map) {
        const int both = boundary.on == 3, none = boundary.on == 0;
        if (both || none || !segment_src || (n_truth == 0 && !boundary.map)) {
            fprintf(stderr, "--boundary-ratio R or --boundary-d N (one of them) needs --segment-source and --truth or --boundary-map; "
                            "--boundary-edge and --boundary-map need one of them\n");
            return 2;
        }
        if ((boundary.on == 1 && !(boundary.ratio > 0.0 && boundary.ratio <= 1.0)) || (boundary.on == 2 && (boundary.d < 1 || boundary.d > MBN_BOUNDARY_MAX_D)) ||
            (boundary.edge != 0 && boundary.edge != 1)) {
            fprintf(stderr, "bad --boundary-ratio (0 < R <= 1), --boundary-d (1 <= N <= %d) or --boundary-edge (0 or 1)\n", MBN_BOUNDARY_MAX_D);
            return 2;
        }
        if (boundary.on == 1) boundary.d = 0;
        boundary.on = n_truth > 0;
    }
    if (surface_on || surface_flags) {
        if (!surface_on || !segment_src || n_truth == 0 || have_topk) {
            fprintf(stderr, "--surface needs --segment-source and --truth and does not go with --segment-topk; --surface-bins, --surface-tolerance, "
                            "--surface-percentile, --surface-edge and --surface-map need --surface\n");
            return 2;
        }
        if (g_surface.bins < 2 || g_surface.bins > MBN_SURFACE_MAX_BINS || g_surface.tolerance < 0 || g_surface.tolerance > g_surface.bins - 2 ||
            !(g_surface.percentile > 0.0 && g_surface.percentile <= 100.0) || (g_surface.edge != 0 && g_surface.edge != 1)) {
            fprintf(stderr, "bad --surface-bins (2 <= N <= %d), --surface-tolerance (0 <= T <= N - 2), --surface-percentile (0 < P <= 100) or "
                            "--surface-edge (0 or 1)\n", MBN_SURFACE_MAX_BINS);
            return 2;
        }
        g_surface.on = 1;
    }
    if (panoptic.on && (!segment_src || n_truth == 0)) {
        fprintf(stderr, "--panoptic needs --segment-source and --truth\n");
        return 2;
    }
    if ((regions.on && !segment_src) || (region_flags && !regions.on && !panoptic.on) || (max_regions_flag && !regions.on)) {
        fprintf(stderr, "--regions needs --segment-source; --connectivity and --min-area need --regions or --panoptic, --max-regions needs --regions\n");
        return 2;
    }
    panoptic.connectivity = regions.connectivity;
    panoptic.min_area = regions.min_area;
    if (panoptic.on && ((panoptic.connectivity != 4 && panoptic.connectivity != 8) || panoptic.min_area < 1)) {
        fprintf(stderr, "bad --connectivity (4 or 8) or --min-area (N >= 1)\n");
        return 2;
    }
    if (regions.on && ((regions.connectivity != 4 && regions.connectivity != 8) || regions.min_area < 1 || regions.max_regions < 0 ||
                       regions.max_regions > MBN_COMPONENTS_MAX_REGIONS)) {
        fprintf(stderr, "bad --connectivity (4 or 8), --min-area (N >= 1) or --max-regions (0 <= M <= %d)\n", MBN_COMPONENTS_MAX_REGIONS);
        return 2;
    }
    if (have_min_conf != have_ignore || (have_min_conf && !segment_src)) {
        fprintf(stderr, "--min-confidence P and --ignore-label L come together and with --segment-source\n");
        return 2;
    }
    if (have_min_conf && (!(min_conf >= 0.f) || !(min_conf <= 1.f) || ignore_label < 0 || ignore_label > 65535)) {
        fprintf(stderr, "bad --min-confidence (0 <= P <= 1) or --ignore-label (0..65535: it is written into the PGM)\n");
        return 2;
    }
    if (out_stride != 0 && out_stride != 8 && out_stride != 16 && out_stride != 32) { fprintf(stderr, "bad --output-stride (32, 16 or 8)\n"); return 2; }
    mbn_context *ctx = NULL;
    if (gpus > 0 && !literal) {
        if (batch < 1 || steps < 1 || warmup < 0 || g_streams < 1 || g_streams > 8) { fprintf(stderr, "bad --batch/--steps/--warmup/--streams\n"); return 2; }
        char tmpm[] = "/tmp/mbn_synth_XXXXXX.h5";
        if (!h5) {
            if (!have_seed) { fprintf(stderr, "need --h5 or --synthetic with --gpus\n"); return 2; }
            int tfd = mkstemps(tmpm, 3);
            if (tfd < 0) { fprintf(stderr, "cannot create a temporary file in /tmp\n"); return 2; }
            close(tfd);
            CHECK(mbn_weights_synthetic_h5(tmpm, alpha > 0.f ? alpha : 1.0f, 1000, seed));
            h5 = tmpm;
        }
        mbn_weights wm;
        CHECK(mbn_weights_from_h5_os(h5, alpha, rows, cols, out_stride, &wm));
        if (h5 == tmpm) remove(tmpm);
        int rc = run_multi(gpus, batch, steps, warmup, &wm, verify);
        mbn_weights_free(&wm);
        return rc;
    }
    printf("Initializing HIP device...\n");
    CHECK(mbn_init(0, &ctx));
    char name[128];
    mbn_device_name(ctx, name, sizeof(name));
    printf("device: %s  (%s)\n", name, mbn_version());
    if (literal) {
        int rc = run_literal(ctx, wfile, image, ref_args);
        mbn_shutdown(ctx);
        return rc;
    }
    char tmp[] = "/tmp/mbn_synth_XXXXXX.h5";
    if (!h5) {
        if (!have_seed) { fprintf(stderr, "need --h5, --synthetic or --literal\n"); return 2; }
        int tfd = mkstemps(tmp, 3);                 /* O_EXCL-created, unpredictable name: no symlink following, no clash between runs */
        if (tfd < 0) { fprintf(stderr, "cannot create a temporary file in /tmp\n"); return 2; }
        close(tfd);
        CHECK(mbn_weights_synthetic_h5(tmp, alpha > 0.f ? alpha : 1.0f, 1000, seed));
        h5 = tmp;
    }
    mbn_weights w;
    CHECK(mbn_weights_from_h5_os(h5, alpha, rows, cols, out_stride, &w));
    if (have_seed) remove(tmp);
    mbn_net *net = NULL;
    const int net_batch = batch > n_views ? batch : n_views;                      /* the views of one image are one batch of the net, and so are its tiles */
    CHECK(mbn_net_create(ctx, &w, net_batch > slide_tiles ? net_batch : slide_tiles, &net));
    CHECK(mbn_net_set_resize_filter(net, filter));
    CHECK(mbn_net_set_pad_color(net, pad_rgb[0], pad_rgb[1], pad_rgb[2]));
    const int classes = w.plan.classes;
    const size_t img = (size_t)rows * cols * 3;          /* [rows][cols][3]: a P6 image cols wide and rows high */
    size_t img_count = (size_t)batch * img;
    unsigned char *u8 = malloc(img_count);
    if (!u8) return 1;
    int pw = 0, ph = 0, have = 0;
    unsigned char *src = NULL;          /* the image at its own size */
    if (ppm && ppm_size(ppm, &pw, &ph) == MBN_OK && pw <= PPM_MAX_SIDE && ph <= PPM_MAX_SIDE && (src = malloc((size_t)pw * ph * 3)) != NULL)
        have = mbn_read_ppm(ppm, src, &pw, &ph, pw * ph) == MBN_OK;
    if (n_ppm > 1) {
        /* files of different sizes: uploaded one behind the other into ONE buffer and resized by one ragged launch; slots n_ppm.. repeat image 0 */
        int64_t *offs = malloc(sizeof(int64_t) * (size_t)n_ppm);
        int32_t *hs = malloc(sizeof(int32_t) * (size_t)n_ppm), *ws = malloc(sizeof(int32_t) * (size_t)n_ppm);
        if (!offs || !hs || !ws) return 1;
        size_t total = 0;
        for (int n = 0; n < n_ppm; n++) {
            if (ppm_size(ppms[n], &pw, &ph) != MBN_OK || pw > PPM_MAX_SIDE || ph > PPM_MAX_SIDE) {
                fprintf(stderr, "%s is not a readable P6 image of at most %d x %d pixels\n", ppms[n], PPM_MAX_SIDE, PPM_MAX_SIDE);
                return 2;
            }
            offs[n] = (int64_t)total; hs[n] = ph; ws[n] = pw;
            total += (size_t)pw * ph * 3;
        }
        unsigned char *all = malloc(total);
        if (!all) return 1;
        for (int n = 0; n < n_ppm; n++) {
            pw = ws[n]; ph = hs[n];
            if (mbn_read_ppm(ppms[n], all + offs[n], &pw, &ph, pw * ph) != MBN_OK) { fprintf(stderr, "cannot read %s\n", ppms[n]); return 2; }
        }
        void *d_src, *d_img;
        CHECK(mbn_alloc(ctx, total, &d_src));
        CHECK(mbn_upload(ctx, d_src, all, total));
        CHECK(mbn_net_resize_inputs(net, d_src, offs, hs, ws, n_ppm, fit, crop_fraction, &d_img));
        CHECK(mbn_download(ctx, u8, d_img, (size_t)n_ppm * img));
        CHECK(mbn_free(ctx, d_src));
        for (int n = n_ppm; n < batch; n++) memcpy(u8 + (size_t)n * img, u8, img);
        for (int n = 0; n < n_ppm; n++)
            printf("image %d: %s, %d wide, %d high, resized to %d x %d (%s)\n", n, ppms[n], ws[n], hs[n], cols, rows, fit_name(fit));
        src_h0 = hs[0]; src_w0 = ws[0];
        free(all); free(offs); free(hs); free(ws);
    } else if (have && pw == cols && ph == rows) {
        for (int n = 0; n < batch; n++) memcpy(u8 + (size_t)n * img, src, img);
    } else if (have) {
        /* any other size: resized on the device into the net's staging buffer; the batch is `batch` copies of that image, as above */
        void *d_src, *d_img;
        CHECK(mbn_alloc(ctx, (size_t)pw * ph * 3, &d_src));
        CHECK(mbn_upload(ctx, d_src, src, (size_t)pw * ph * 3));
        CHECK(mbn_net_resize_input(net, d_src, 1, ph, pw, fit, crop_fraction, &d_img));
        CHECK(mbn_download(ctx, u8, d_img, img));
        CHECK(mbn_free(ctx, d_src));
        for (int n = 1; n < batch; n++) memcpy(u8 + (size_t)n * img, u8, img);
        printf("image: %s, %d wide, %d high, resized to %d x %d (%s)\n", ppm, pw, ph, cols, rows, fit_name(fit));
        src_h0 = ph; src_w0 = pw;
    } else {
        if (ppm) fprintf(stderr, "warning: %s is not a readable P6 image of at most %d x %d pixels; using a synthetic one\n", ppm, PPM_MAX_SIDE, PPM_MAX_SIDE);
        unsigned long long s = 0xC0FFEEULL;
        for (size_t i = 0; i < img_count; i++) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; u8[i] = (unsigned char)(s >> 56); }
    }
    free(src);
    void *d_u8, *d_logits, *d_probs, *d_arg;
    CHECK(mbn_alloc(ctx, img_count, &d_u8));
    CHECK(mbn_alloc(ctx, (size_t)batch * classes * sizeof(float), &d_logits));
    CHECK(mbn_alloc(ctx, (size_t)batch * classes * sizeof(float), &d_probs));
    CHECK(mbn_alloc(ctx, (size_t)batch * 8 * sizeof(int), &d_arg));
    CHECK(mbn_upload(ctx, d_u8, u8, img_count));
    CHECK(mbn_net_set_input_u8(net, 1));   /* layer 1 reads the raw image and applies the Keras x/127.5 - 1 at load */
    float ms[MBN_MAX_LAYERS];
    CHECK(mbn_net_forward_timed(net, d_u8, d_logits, batch, ms, MBN_MAX_LAYERS));
    for (int i = 0; i < w.plan.n_layers; i++) {
        if (w.plan.layer[i].kind == MBN_L_FC) printf("Kernel Execution time for Fully Connected Layer: %f\n", ms[i] / 1000.0);
        else printf("Kernel Execution time for Layer %d: %f\n", i + 1, ms[i] / 1000.0);
    }
    /* classifier read-out on the device: only the 5 best (index, probability) pairs per image cross PCIe, instead of the
     * reference's 1000 logits + host exp loop (MobileNet.c:2744-2792) */
    const int topk = classes < 5 ? classes : 5;
    CHECK(mbn_softmax_topk_f32(ctx, NULL, d_arg, d_probs, d_logits, batch, classes, topk, NULL));
    int *arg = malloc(sizeof(int) * (size_t)batch * topk);
    float *probs = malloc(sizeof(float) * (size_t)batch * topk);
    if (!arg || !probs) return 1;
    CHECK(mbn_download(ctx, arg, d_arg, sizeof(int) * (size_t)batch * topk));
    CHECK(mbn_download(ctx, probs, d_probs, sizeof(float) * (size_t)batch * topk));
    printf("Highest Probability of the element is present at location %d and it's value is %f.\n", arg[0] + 1, probs[0]);
    printf("top-%d:", topk);
    for (int j = 0; j < topk; j++) printf(" %d (%f)", arg[j] + 1, probs[j]);
    printf("\n");
    for (int n = 0; n_ppm > 1 && n < n_ppm; n++) printf("top-1 of image %d (%s): %d (%f)\n", n, ppms[n], arg[n * topk] + 1, probs[n * topk]);
    if (segment) {
        void *d_labels;
        int *labels = malloc(sizeof(int) * (size_t)rows * cols);
        if (!labels) return 1;
        CHECK(mbn_alloc(ctx, sizeof(int) * (size_t)batch * rows * cols, &d_labels));
        CHECK(mbn_net_segment(net, d_u8, batch, d_labels, NULL));
        CHECK(mbn_download(ctx, labels, d_labels, sizeof(int) * (size_t)rows * cols));
        const int bad = write_label_map(segment, labels, rows, cols, classes, -1, "");
        free(labels);
        if (bad) return 1;
        int32_t rect[4];
        if (fit == MBN_FIT_PAD && src_h0 > 0 && mbn_fit_pad(src_h0, src_w0, rows, cols, rect) == MBN_OK)
            printf("segment: image 0 is the %d x %d rectangle at (%d, %d) of the label map (wide x high, left, upper); the rest labels the border\n", rect[2],
                   rect[3], rect[0], rect[1]);
    }
    if (have_topk) {
        const int bad = segment_source_topk(ctx, net, ppm, segment_src, classes, fit, segment_topk, segment_conf, min_conf, have_ignore ? ignore_label : -1,
                                            n_truth ? truths[0] : NULL);
        if (bad) return bad;
    } else if (segment_src || segment_conf) {
        const int bad = segment_source(ctx, net, ppms, n_ppm, segment_src, classes, fit, segment_conf, min_conf, have_ignore ? ignore_label : -1,
                                       view_scales, view_mirrors, n_views, slide_tiles ? slide : NULL, truths, n_truth, &regions, &boundary, &panoptic);
        if (bad) return bad;
    }
    mbn_net_destroy(net);
    mbn_weights_free(&w);
    mbn_shutdown(ctx);
    free(u8); free(arg); free(probs); free(ppms); free(truths);
    return 0;
}
